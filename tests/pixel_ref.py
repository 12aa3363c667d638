"""The pixel stage of the augmentation (csrc/diffaug.hip: sgx_diffaug, sgx_diffaug_gated, sgx_diffaug_blit) held per element: an fp64
restatement in the kernels' own layout ([B][H][W][3]) built on the parameters of tests/diffaug_ref.py and tests/blit_ref.py, which
elements must come out bit for bit, a two-term bound for the others, inputs and draws that reach the seams, and the table of rows
(CASES) that tests/test_gpu_pixel_paths.py runs and tests/test_pixel_coverage.py holds to the launch sites.  Test-side only: nothing
here calls the library.

The criterion.  An image whose effective bits lack colour is gathers and zeros: every element equals the fp32 input it gathers, or
+0.0 (sign bit clear) where the shift leaves the image or the cutout masks -- ``exact``.  So are the forward-masked elements of a
colour image (+0.0; the mask comes after the colour).  Every other element of a colour image is

    o = cs (v - m) + c m + (1 - c) M + b,   m = (v0 + v1 + v2) / 3,  M = the image mean of what the sum pass sums

and the kernels' fp32 value is within

    (n_M + 2) u |1 - c| M_abs  +  (n_r + 2) u S_r,        u = 2^-24
    S_r = |c s| (|v| + m_abs) + |c| m_abs + |1 - c| M_abs + |b|

of it, M_abs the image mean of |x| (adjoint: of |G^T Shift^T Mask g|), m_abs the pixel's mean of |v|.  (+ 2: the second-order terms
and the fp32 rounding of the inputs' fp64 expression, as streaming_ref.assert_elementwise.)

n_M, the longest fp32 chain behind M (diffaug_sum_kernel / diffaug_blit_sum_kernel, then the finishing loop of diffaug_apply_kernel /
da_blit_mean): 3P adds into a unit's s, UPT = 16384 / (256 P) adds into a thread's acc, 6 steps of wave_sum, 3 adds over the block's
four waves, ceil(nparts / 64) adds of the lane-strided finishing loop, 6 steps of wave_sum, the quotient by 3 H W (exact as a product
for every shape here: 3 H W < 2^24) and the product with 1 - c (exact from the fp32 c): 46 at P = 4 and 85 at P = 1 up to 64 partials.

The colour parameters are the fp32 numbers the kernels hold: b = u0 - 0.5f and c = u2 + 0.5f, each one fp32 operation on an fp32 draw
(``params_of``), s = 2 u1 (exact); the reference evaluates the expression above on them in fp64.  (With c = u2 + 0.5 in fp64 instead, the
rounding of c would move (1 - c) M by up to u |M|, which no term of the bound covers once |1 - c| is below about 1 / 60 and the pixel is
small against the mean.)  1 - c is then exact in fp32: c is a multiple of 2^-24 in [0.5, 1) and of 2^-23 in [1, 1.5].

n_r = 8, the longest chain from v to the store, through cs (v - m): m is two adds, the product with 1.f / 3.f and that constant's own
rounding (4); v - m (5); cs = c s rounded (6); the product (7); + cm (8).  The other terms are shorter: c m is 4 + the product + two
adds = 7, (1 - c) M after n_M is + b, + c m, the last add = 3, b the same three adds.  A contraction of a product and an add into an
fma only removes roundings.
The bound carries no measured margin.  Worst err / bound: the numpy fp32 emulation of tests/test_pixel_coverage.py 0.27 on the rows up
to 132 x 132 and 0.40 at 1028 x 1028; the kernels on an MI355X 0.45 (the adjoint at 1028 x 1028), the same for all three entries."""
import collections

import numpy as np

import blit_ref as Bl                                        # (its parameters are diffaug_ref.params plus f and k)

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
N_R = 8
BLOCK, PART_PIXELS, WAVE = 256, 16384, 64
COLOR, TRANSLATION, CUTOUT, XFLIP, ROT90 = 1, 2, 4, 8, 16
MODES = ((0, 1), (0, 0), (1, 0))                             # (adjoint, with_bias): forward, its linear part, adjoint
MODE_NAME = {(0, 1): "fwd", (0, 0): "lin", (1, 0): "adj"}
DIFFAUG, GATED, BLIT = "sgx_diffaug", "sgx_diffaug_gated", "sgx_diffaug_blit"
KERNELS = ("diffaug_sum_kernel", "diffaug_apply_kernel", "diffaug_blit_sum_kernel", "diffaug_blit_row_kernel", "diffaug_blit_tile_kernel")
CONTROLLER = {"sgx_ada_gates": "ada_gates_kernel", "sgx_ada_gates_n": "ada_gates_n_kernel", "sgx_ada_update": "ada_update_kernel"}
INSTANTIATIONS = 26                                          # sum 8, apply 8, blit sum 4, blit row 4, tile 2


def cdiv(a, b):
    return -(-a // b)


def nparts(H, W):
    return cdiv(H * W, PART_PIXELS)


def pixels_per_lane(W, off):
    return 4 if W % 4 == 0 and off == 0 else 1


def n_M(P, parts):
    return 3 * P + PART_PIXELS // (BLOCK * P) + 6 + 3 + cdiv(parts, WAVE) + 6 + 2


def kernels_of(entry, H, W, off, policy, adjoint):
    """The instantiations a call launches, as the source spells them (da_plan restated)."""
    P, tf = pixels_per_lane(W, off), lambda v: "true" if v else "false"
    blit, gated, mode = entry == BLIT, entry == GATED, 2 if adjoint else 0
    out = []
    if policy & COLOR:
        out.append(f"diffaug_blit_sum_kernel<{P}, {mode}>" if blit else f"diffaug_sum_kernel<{P}, {mode}, {tf(gated)}>")
    if blit and P == 4 and policy & ROT90:
        out.append(f"diffaug_blit_tile_kernel<{tf(adjoint)}>")
    elif blit:
        out.append(f"diffaug_blit_row_kernel<{P}, {tf(adjoint)}>")
    else:
        out.append(f"diffaug_apply_kernel<{P}, {tf(adjoint)}, {tf(gated)}>")
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- the index maps
def g_inv(a, b, f, k, H, W):
    """G(x)[a][b] = x[g_inv(a, b)], G = Rot^k o Flip (include/sgx.h; k odd needs H == W): the turn's rule, then the flip's."""
    if k == 1:
        a, b = b, H - 1 - a
    elif k == 2:
        a, b = H - 1 - a, W - 1 - b
    elif k == 3:
        a, b = W - 1 - b, a
    return (a, W - 1 - b) if f else (a, b)


def g_fwd(i, j, f, k, H, W):
    """Where input pixel (i, j) lands under G: the inverse of g_inv, the flip undone first."""
    if f:
        j = W - 1 - j
    if k == 1:
        return H - 1 - j, i
    if k == 2:
        return H - 1 - i, W - 1 - j
    if k == 3:
        return j, W - 1 - i
    return i, j


def index_map(p, H, W, adjoint, cut_at_output=False):
    """-> (si, sj, ok) [H][W]: the source pixel of every output pixel and whether it has one.  Forward: the shifted position
    (i + tx, j + ty) inside the image, no cutout at the OUTPUT pixel, source G^-1 of the shifted position.  Adjoint: (a, b) = G(i, j),
    source (a - tx, b - ty) inside the image and outside the cutout (tested at the SOURCE).  ``cut_at_output``: the planted error."""
    i, j = np.mgrid[0:H, 0:W]
    cut = lambda r, c: (r >= p["r0"]) & (r < p["r1"]) & (c >= p["c0"]) & (c < p["c1"])
    inside = lambda r, c: (r >= 0) & (r < H) & (c >= 0) & (c < W)
    if adjoint:
        a, b = g_fwd(i, j, p["f"], p["k"], H, W)
        si, sj = a - p["tx"], b - p["ty"]
        ok = inside(si, sj) & ~(cut(i, j) if cut_at_output else cut(si, sj))
    else:
        a, b = i + p["tx"], j + p["ty"]
        ok = inside(a, b) & ~cut(i, j)
        si, sj = g_inv(a, b, p["f"], p["k"], H, W)
    return si, sj, ok


def gather(xb, si, sj, ok):
    H, W, _ = xb.shape
    v = xb[np.clip(si, 0, H - 1), np.clip(sj, 0, W - 1)]
    return np.where(ok[..., None], v, xb.dtype.type(0))


def params_of(u_row, H, W, bits):
    """blit_ref.params9 for a row of seven or nine draws."""
    row = list(u_row) + [0.0, 0.0] if len(u_row) == 7 else list(u_row[:9])
    p = Bl.params9(row, H, W, bits)
    if bits & COLOR:                                         # b and c as the kernels hold them: one fp32 operation each
        p.update(b=float(f32(row[0]) - f32(0.5)), c=float(f32(row[2]) + f32(0.5)))
    return p


# ---------------------------------------------------------------------------------------------------------------- reference and bound
def reference(x, u, bits, adjoint, with_bias, P):
    """x fp64 [B][H][W][3], u [B][7 or 9], bits [B] (an image's effective bits) -> (ref fp64, exact bool, bound fp64), all [B][H][W][3].
    ``P``: the pixels per lane of the launch (it sets n_M)."""
    B, H, W, _ = x.shape
    ref, exact, bound = np.zeros_like(x), np.ones(x.shape, bool), np.zeros_like(x)
    nm = n_M(P, nparts(H, W))
    for n in range(B):
        p = params_of(u[n], H, W, bits[n])
        si, sj, ok = index_map(p, H, W, adjoint)
        v = gather(x[n], si, sj, ok)
        if not bits[n] & COLOR:
            ref[n] = v
            continue
        summed = v if adjoint else x[n]
        M, M_abs = summed.mean(), np.abs(summed).mean()
        m, m_abs = v.mean(-1, keepdims=True), np.abs(v).mean(-1, keepdims=True)
        c, s, b = p["c"], p["s"], (p["b"] if with_bias and not adjoint else 0.0)
        o = c * s * (v - m) + c * m + (1 - c) * M + b
        S = abs(c * s) * (np.abs(v) + m_abs) + abs(c) * m_abs + abs(1 - c) * M_abs + abs(b)
        live = np.ones_like(ok) if adjoint else ok
        ref[n] = np.where(live[..., None], o, 0.0)
        exact[n] = ~live[..., None]
        bound[n] = (nm + 2) * U * abs(1 - c) * M_abs + (N_R + 2) * U * S
    return ref, exact, bound


def check(y, ref, exact, bound, what=""):
    """y fp32 [B][H][W][3] (numpy): the exact elements bit for bit against ref rounded to fp32 (ref is an fp32 input or +0.0 there), the
    others within the bound; a NaN fails either.  The first offender is named.  -> the worst err / bound."""
    y = np.ascontiguousarray(y, f32)
    assert y.shape == ref.shape == exact.shape == bound.shape, (what, y.shape, ref.shape)
    want = np.ascontiguousarray(ref.astype(f32))
    bad = exact & (y.view(np.int32) != want.view(np.int32))
    if bad.any():
        at = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {int(exact.sum())} exact elements differ in bits; first at (b, i, j, ch) = {at}: got {float(y[at])!r} "
                             f"(0x{int(y.view(np.uint32)[at]):08x}), want {float(want[at])!r} (0x{int(want.view(np.uint32)[at]):08x})")
    err = np.abs(y.astype(f64) - ref)
    bad = ~exact & ~(err <= bound)
    if bad.any():
        at = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {int((~exact).sum())} elements outside the bound; first at (b, i, j, ch) = {at}: got {float(y[at])!r}, "
                             f"ref {float(ref[at])!r}, err {float(err[at]):.3e} > bound {float(bound[at]):.3e}")
    live = ~exact & (bound > 0)
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def old_criterion(y, ref):
    """What tests/test_gpu_diffaug.py, test_gpu_ada.py and test_gpu_blit.py (colour images) ask: one number for the batch."""
    err, tol = float(np.abs(y.astype(f64) - ref).max()), 1e-5 * float(np.abs(ref).max()) + 1e-30
    return err, tol, bool(err <= tol)


# ---------------------------------------------------------------------------------------------------------------- inputs and draws
def images(B, H, W, seed, colour=True):
    """fp32 [B][H][W][3].  ``colour``: every image a mean of the order of its spread, different per image, the amplitudes of a batch
    from 1e-3 to 1e3 (B = 1: 1); else randn."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, H, W, 3))
    if colour:
        amp = 10.0 ** (np.linspace(-3, 3, B) if B > 1 else np.zeros(1))
        mean = np.array([(0.5 + n % 3) * (-1) ** n for n in range(B)])
        x = (x + mean[:, None, None, None]) * amp[:, None, None, None]
    return x.astype(f32)


def amplitudes(x):
    return np.abs(x.astype(f64)).mean(axis=(1, 2, 3))


def u_for(value, n):
    """A uniform whose draw min(floor(u n), hi) is ``value``: the middle of its cell."""
    return f32((value + 0.5) / n)


ROWS_OF = {8: list(range(8)), 5: [0, 1, 5, 6, 7], 3: [0, 7, 5], 2: [5, 7], 1: [5]}
SIGNS = ((-1, -1), (1, 1), (1, -1), (-1, 1), (1, -1), (-1, -1), (-1, 1), (1, 1))
DESIGNED = {2: 0, 4: 1, 5: 2, 6: 3}                          # the rows whose cutout is placed: row -> c0 % 4 (before the variant turns it)


def draws(B, H, W, variant=0, seed=0):
    """[B][9] fp32: blit_ref.edge_draws9(8) (rows 0..3 the edges of u0..u6, rows 0..7 the eight orientations), and
      row 7: u = 1.0 in every column (row 0 is u = 0.0 in every column), both at variant 0;
      every row's translation at (+-sh, +-sw) with the signs of SIGNS (u = 0.0, 1 - 2^-24 or 1.0), negated by ``variant`` 1: over
      the two variants every orientation is shifted out on all four sides;
      rows 2, 4, 5, 6: the cutout's first column c0 = 0, 1, 2, 3 (mod 4; + variant) with the box inside the row where the width
      allows it (c1 = c0 + cw runs through the residues with it), its first row spread over the height.
    B < 8 takes the rows ROWS_OF[B]."""
    u = Bl.edge_draws9(8, seed).copy()
    u[7, :] = f32(1.0)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    nx, ny = H + 1 - ch % 2, W + 1 - cw % 2
    for r in range(8):
        sx, sy = SIGNS[r]
        if variant:
            sx, sy = -sx, -sy
        hi = f32(1.0) if r == 7 else f32(Bl.EDGE)
        u[r, 3], u[r, 4] = (hi if sx > 0 else f32(0.0)), (hi if sy > 0 else f32(0.0))
        if r in DESIGNED:
            c0 = (DESIGNED[r] + variant) % 4
            r0 = (5 * r + 1) % max(H - ch + 1, 1)
            u[r, 5], u[r, 6] = u_for(min(r0 + ch // 2, nx - 1), nx), u_for(min(c0 + cw // 2, ny - 1), ny)
    return u[ROWS_OF[B]].astype(f32)


# B = 8, by the variant of the draws: at variant 0 the row of zeros (0) has every op and the row of ones (7) translation and cutout; at
# variant 1 the four rows whose cutout is placed (2, 4, 5, 6) have the cutout bit
GATES3 = {8: ((7, 0, 1, 2, 3, 4, 5, 6), (1, 2, 4, 3, 5, 6, 7, 0)), 5: (7, 0, 6, 1, 5), 3: (7, 0, 6), 2: (7, 6), 1: (7,)}
HIGH = {8: (24, 0, 0, 24, 16, 8, 24, 16), 5: (24, 0, 8, 16, 24), 3: (24, 0, 16), 2: (8, 24), 1: (24,)}


def gates_of(entry, B, policy, variant=0):
    """The per-image bits of a gated row: every pattern of the three ops at B = 8 (0 among them: a copy), and for the blit entry
    the two orientation bits on and off beside them; always a subset of the policy."""
    low = GATES3[B][variant] if B == 8 else GATES3[B]
    if entry == BLIT:
        return [policy & (l | h) if l else 0 for l, h in zip(low, HIGH[B])]
    return [policy & l for l in low]


# ---------------------------------------------------------------------------------------------------------------- the rows
Case = collections.namedtuple("Case", "id entry args kernels why")
CASES = []


def _row(entry, B, H, W, off, policy, mode, gated, why, variant=0, wide=0):
    adjoint, with_bias = mode
    id = f"{entry[4:]}-B{B}-{H}x{W}{'+%d' % off if off else ''}-p{policy}-{MODE_NAME[mode]}{'-gated' if gated else ''}{'-wide' if wide else ''}{'-v1' if variant else ''}"
    args = dict(B=B, H=H, W=W, off=off, policy=policy, adjoint=adjoint, with_bias=with_bias, gated=gated, variant=variant, wide=wide)
    CASES.append(Case(id, entry, args, kernels_of(entry, H, W, off, policy, adjoint), why))


def _three(B, H, W, off, policies, why, modes=MODES, both_variants=False):
    """``both_variants``: the gated rows with either set of draws and gates."""
    for policy in policies:
        for mode in modes:
            _row(DIFFAUG, B, H, W, off, policy, mode, False, why)
            _row(GATED, B, H, W, off, policy, mode, True, why, variant=1)
            if both_variants:
                _row(GATED, B, H, W, off, policy, mode, True, why, variant=0)


def _blit(B, H, W, off, policies, why, modes=MODES, both_variants=False, both_gated=False):
    for n, policy in enumerate(policies):
        for k, mode in enumerate(modes):
            _row(BLIT, B, H, W, off, policy, mode, False, why, variant=0, wide=(n + k) % 2)
            _row(BLIT, B, H, W, off, policy, mode, True, why, variant=1, wide=(n + k + 1) % 2)
            if both_variants:
                _row(BLIT, B, H, W, off, policy, mode, False, why, variant=1, wide=(n + k + 1) % 2)
            if both_gated:
                _row(BLIT, B, H, W, off, policy, mode, True, why, variant=0, wide=(n + k) % 2)


SQUARE = (31, 30, 24, 25, 8, 16, 1, 0)                       # test_gpu_blit.SQUARE plus 1 and 0
FLAT = (15, 14, 8, 9, 1, 0)                                  # not square: no rot90
ALL3 = (1, 2, 3, 4, 5, 6, 7)

for B_, H_, W_ in ((3, 1, 1), (3, 1, 5), (3, 3, 2), (3, 2, 3)):
    why = "H or W below 4: sh = sw = 0 on that side, the cutout is one row / column or the whole image, W = 1"
    _three(B_, H_, W_, 0, (7, 6), why)
    _blit(B_, H_, W_, 0, (31, 30) if H_ == W_ else (15, 14), why)
for B_, H_, W_, off_, why in ((8, 4, 4, 0, "one block, P = 4, the smallest image of whole groups"), (8, 5, 7, 0, "one block, P = 1 by width, ch odd"),
                              (8, 9, 12, 0, "one block, P = 4 by width, ch odd / cw even"), (8, 6, 10, 0, "one block, P = 1 by width, ch odd, cw odd"),
                              (8, 16, 16, 1, "one block, P = 1 by alignment (a base one float off)")):
    _three(B_, H_, W_, off_, ALL3, why, both_variants=True)
    _blit(B_, H_, W_, off_, SQUARE if H_ == W_ else FLAT, why + ("; the tile kernel on one tile that is mostly overhang" if (H_, off_) == (4, 0) else ""), both_gated=True)
_three(5, 36, 36, 0, (7, 6), "two apply blocks, the second ragged: 324 units at P = 4")
_three(5, 17, 17, 0, (7, 6), "two apply blocks, the second ragged: 289 units at P = 1")
_blit(5, 36, 36, 0, (15, 14), "the row kernel on two blocks, 324 units at P = 4")
_blit(5, 17, 17, 0, (31, 30), "the row kernel per pixel on two blocks (rot90 without whole groups)")
for H_, W_, why in ((128, 128, "exactly one full partial"), (128, 132, "two partials, P = 4, the second ragged"), (127, 131, "two partials, P = 1")):
    _three(2, H_, W_, 0, (7, 6), why)
    _blit(2, H_, W_, 0, (15, 14), why + ", the blit sum pass and the row kernel")
_blit(2, 132, 132, 0, (31, 30), "the tile kernel with two partials per image")
for N_, why in ((8, "one tile, mostly overhang"), (32, "exactly one tile"), (36, "2 x 2 tiles with overhang"), (64, "2 x 2 tiles, no overhang")):
    _blit(8, N_, N_, 0, SQUARE if N_ == 8 else (31, 30), "the tile kernel: " + why + "; all eight orientations in one launch, shifted out on every side", both_variants=True)
for mode_ in ((0, 1), (1, 0)):
    why = "65 partials: the second trip of the lane-strided finishing loop"
    _row(DIFFAUG, 1, 1028, 1028, 0, 7, mode_, False, why)
    _row(GATED, 1, 1028, 1028, 0, 7, mode_, True, why)
    _row(BLIT, 1, 1028, 1028, 0, 31, mode_, False, why + " of da_blit_mean, tile kernel")
    _row(BLIT, 1, 1028, 1028, 0, 15, mode_, False, why + " of da_blit_mean, row kernel")
for entry_, where in (("sgx_ada_gates", "tests/test_gpu_ada.py::test_gates_kernel_vs_restatement"), ("sgx_ada_gates_n", "tests/test_gpu_blit.py::test_gates_n_kernel_vs_restatement"),
                      ("sgx_ada_update", "tests/test_gpu_ada.py::test_controller_kernel_vs_restatement")):
    CASES.append(Case(entry_[4:] + "-B7", entry_, dict(B=7, runs=where), (CONTROLLER[entry_],), "one-dimensional, outside the plan; bit for bit against its fp32 restatement, also at B = 1 and 1000 in " + where))
BY_ID = {c.id: c for c in CASES}
IMAGE_CASES = [c for c in CASES if c.entry in (DIFFAUG, GATED, BLIT)]
LARGE = [c for c in IMAGE_CASES if c.args["H"] > 132]


def effective_bits(c):
    a = c.args
    return gates_of(c.entry, a["B"], a["policy"], a["variant"]) if a["gated"] else [a["policy"]] * a["B"]


def inputs(c):
    """-> (x fp32 [B][H][W][3], u fp32 [B][9]) of a row; x is the image, or for an adjoint row the incoming gradient."""
    a = c.args
    seed = 1000 * a["H"] + 10 * a["W"] + a["adjoint"]
    return images(a["B"], a["H"], a["W"], seed, bool(a["policy"] & COLOR)), draws(a["B"], a["H"], a["W"], a["variant"], seed=a["H"] + a["W"])


def expected(c, x=None, u=None):
    """reference() of a row on its own inputs."""
    a = c.args
    if x is None:
        x, u = inputs(c)
    return reference(x.astype(f64), u, effective_bits(c), a["adjoint"], a["with_bias"], pixels_per_lane(a["W"], a["off"]))
