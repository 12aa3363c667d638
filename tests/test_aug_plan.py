"""CPU: what a call of an augmentation image pass will launch, asked of the library itself.  sgx_aug_plan answers from da_plan / dg_plan /
dc_plan, the functions the five entry points of csrc/diffaug.hip, adageom.hip and adacolor.hip execute, so on both sides of every seam --
rows that do and do not split into groups of four, aligned and offset bases, the colour pass's rule on H W instead of W, the sum pass with
and without the colour bit and with one and two partials, the three blit paths, one and two blocks or tiles, tile grids that are not
square, the batch as grid y, the three (adjoint, with_bias) modes -- (a) kernel, template arguments, grid and geometry arguments are
what tests/aug_ref.py restates, and what this file states by value; (b) sgx_diffaug_ws_bytes is 4 B nparts of the query; (c) what an
entry rejects, an unknown entry and a NULL out are rejected with the entry's code; (d) the three files have one launch site per kernel,
14 in all.  The query is host-only: nothing here launches."""
import collections
import itertools
import os
import re

import pytest

import aug_ref as AR
import test_streaming_coverage as TSC
from aug_ref import BLIT, COLOR, DIFFAUG, GATED, GEOM, Launch

FILES = ("diffaug.hip", "adageom.hip", "adacolor.hip")
MODES = ((0, 1), (0, 0), (1, 0))                             # (adjoint, with_bias): forward, linear part, adjoint
SIZES = ((5, 7), (2, 6), (3, 6), (16, 16), (30, 30), (32, 32), (36, 36), (33, 64), (8, 96), (128, 128), (132, 132))
MASK = {DIFFAUG: 7, GATED: 7, BLIT: 31}


@pytest.fixture(scope="module")
def lib():
    from stylegan.pytorch_amd import native
    native.build()
    return native.lib()


def test_the_query_is_the_restated_plan_on_both_sides_of_every_seam(lib):
    n = 0
    for (H, W), B, aligned, (adjoint, with_bias) in itertools.product(SIZES, (1, 5), (0, 1), MODES):
        for entry in (DIFFAUG, GATED, BLIT):
            for bits in range(MASK[entry] + 1):
                if bits & AR.ROT90_BIT and H != W:
                    continue
                got = AR.lib_plan(lib, entry, B, H, W, bits, adjoint, with_bias, aligned)
                assert got == AR.plan(entry, B, H, W, bits, adjoint, with_bias, aligned), (entry, B, H, W, bits, adjoint, aligned, got)
                assert all(l.gy == B and l.gx >= 1 for l in got)
                n += 1
        assert AR.lib_plan(lib, GEOM, B, H, W, 0, adjoint, 0, aligned) == AR.plan(GEOM, B, H, W, 0, adjoint, 0, aligned), (B, H, W, adjoint, aligned)
        assert AR.lib_plan(lib, COLOR, B, H, W, 0, adjoint, with_bias, aligned) == AR.plan(COLOR, B, H, W, 0, adjoint, with_bias, aligned), (B, H, W, adjoint, with_bias, aligned)
    assert n > 5000


def one(lib, *a, **kw):
    got = AR.lib_plan(lib, *a, **kw)
    assert len(got) == 1, got
    return got[0]


def test_the_seams_by_value(lib):
    """The table of the seams, each side stated here (not through aug_ref.plan)."""
    ids = lambda *a, **kw: AR.launches_of(AR.lib_plan(lib, *a, **kw))[0]
    # the vector rule: rows of whole groups of four AND aligned bases
    for entry, vec_k, px_k in ((DIFFAUG, AR.APPLY, AR.APPLY), (GATED, AR.APPLY, AR.APPLY), (BLIT, AR.BLIT_ROW, AR.BLIT_ROW), (GEOM, AR.GEOM_TILE, AR.GEOM_PX)):
        bits = 0 if entry == GEOM else 2
        for H, W, aligned, vec in ((32, 32, 1, True), (30, 30, 1, False), (32, 32, 0, False), (30, 30, 0, False)):
            l = one(lib, entry, 1, H, W, bits, 0, 1, aligned)
            assert l.kernel == (vec_k if vec else px_k) and (entry == GEOM or l.P == (4 if vec else 1)), (entry, H, W, aligned, l)
            if entry != GEOM:
                assert l.gx == AR.cdiv(H * W // (4 if vec else 1), 256)
    # the colour pass asks H W % 4, the others W % 4
    assert one(lib, COLOR, 1, 2, 6, 0, 0, 1, 1) == Launch(AR.COLOR_VEC, 0, 0, 0, 1, 1, 1, 0, 0, 12)
    assert one(lib, COLOR, 1, 3, 6, 0, 0, 1, 1) == Launch(AR.COLOR_PX, 0, 0, 0, 1, 1, 1, 0, 0, 18)
    assert one(lib, COLOR, 1, 2, 6, 0, 0, 1, 0).kernel == AR.COLOR_PX
    for H in (2, 3):
        assert one(lib, DIFFAUG, 1, H, 6, 2).P == 1 and one(lib, BLIT, 1, H, 6, 8).P == 1 and one(lib, GEOM, 1, H, 6).kernel == AR.GEOM_PX
    # the sum pass: with the colour bit only, first; 16384 pixels per partial
    for entry, k_sum in ((DIFFAUG, AR.SUM), (GATED, AR.SUM), (BLIT, AR.BLIT_SUM)):
        assert [l.kernel for l in AR.lib_plan(lib, entry, 2, 128, 128, 7)][:-1] == [k_sum] and len(AR.lib_plan(lib, entry, 2, 128, 128, 6)) == 1
        for N, parts in ((128, 1), (132, 2)):
            s, a = AR.lib_plan(lib, entry, 2, N, N, 7)
            assert (s.gx, s.gy, s.nparts, a.nparts) == (parts, 2, parts, parts), (entry, N, s, a)
            assert lib.sgx_diffaug_ws_bytes(2, N, N) == 4 * 2 * s.nparts
    # blit: tile with rot90 and vec, row without rot90, the row kernel per pixel without vec (with and without rot90)
    assert ids(BLIT, 1, 32, 32, 31, 0, 1, 1) == ["diffaug_blit_sum_kernel<4, 0>", "diffaug_blit_tile_kernel<false>"]
    assert ids(BLIT, 1, 32, 32, 15, 0, 1, 1) == ["diffaug_blit_sum_kernel<4, 0>", "diffaug_blit_row_kernel<4, false>"]
    assert ids(BLIT, 1, 32, 32, 31, 1, 0, 0) == ["diffaug_blit_sum_kernel<1, 2>", "diffaug_blit_row_kernel<1, true>"]
    assert ids(BLIT, 1, 30, 30, 16, 0, 1, 1) == ["diffaug_blit_row_kernel<1, false>"]
    assert [AR.note_name(l) for l in AR.lib_plan(lib, BLIT, 1, 30, 30, 31)] == ["diffaug_blit_sum", "diffaug_blit_px"]
    for N, t in ((32, 1), (36, 2)):
        l = one(lib, BLIT, 3, N, N, 16)
        assert l == Launch(AR.BLIT_TILE, 0, 0, 0, 0, t * t, 3, 1, t, 0), (N, l)
    # the apply grid: one unit (four pixels) per thread
    assert one(lib, DIFFAUG, 1, 16, 16, 6).gx == 1 and one(lib, DIFFAUG, 1, 36, 36, 6).gx == 2 and one(lib, BLIT, 1, 36, 36, 8).gx == 2
    assert one(lib, COLOR, 1, 36, 36).gx == 2 and one(lib, COLOR, 1, 16, 16).gx == 1 and one(lib, COLOR, 1, 36, 36, aligned=0).gx == 6
    # geom's tile grid where it is not square: tiles per row is the WIDTH's
    assert one(lib, GEOM, 1, 33, 64) == Launch(AR.GEOM_TILE, 0, 0, 0, 0, 4, 1, 0, 2, 0)
    assert one(lib, GEOM, 1, 8, 96, adjoint=1) == Launch(AR.GEOM_TILE, 0, 1, 0, 0, 3, 1, 0, 3, 0)
    assert one(lib, GEOM, 1, 96, 8) == Launch(AR.GEOM_TILE, 0, 0, 0, 0, 3, 1, 0, 1, 0)
    assert one(lib, GEOM, 1, 33, 63) == Launch(AR.GEOM_PX, 0, 0, 0, 0, AR.cdiv(33 * 63, 256), 1, 0, 0, 0)
    # the batch is grid y
    for entry in (DIFFAUG, GATED, BLIT, GEOM, COLOR):
        for B in (1, 5, 65535):
            assert [l.gy for l in AR.lib_plan(lib, entry, B, 8, 8, 1 if entry < GEOM else 0)] == [B] * (2 if entry < GEOM else 1)
    # the template arguments of the three (adjoint, with_bias) modes, as the launchers' if-ladders chose them
    want = {DIFFAUG: {(0, 1): ["diffaug_sum_kernel<4, 0, false>", "diffaug_apply_kernel<4, false, false>"], (1, 0): ["diffaug_sum_kernel<4, 2, false>", "diffaug_apply_kernel<4, true, false>"]},
            GATED: {(0, 1): ["diffaug_sum_kernel<4, 0, true>", "diffaug_apply_kernel<4, false, true>"], (1, 0): ["diffaug_sum_kernel<4, 2, true>", "diffaug_apply_kernel<4, true, true>"]},
            BLIT: {(0, 1): ["diffaug_blit_sum_kernel<4, 0>", "diffaug_blit_tile_kernel<false>"], (1, 0): ["diffaug_blit_sum_kernel<4, 2>", "diffaug_blit_tile_kernel<true>"]},
            GEOM: {(0, 1): ["ada_geom_tile_kernel<false>"], (1, 0): ["ada_geom_tile_kernel<true>"]},
            COLOR: {(0, 1): ["ada_color_vec_kernel<false, true>"], (0, 0): ["ada_color_vec_kernel<false, false>"], (1, 0): ["ada_color_vec_kernel<true, false>"]}}
    for entry, by_mode in want.items():
        for adjoint, with_bias in MODES:
            k = by_mode[(adjoint, with_bias)] if (adjoint, with_bias) in by_mode else by_mode[(0, 1)]      # only the colour pass has a BIAS argument
            assert ids(entry, 2, 32, 32, MASK.get(entry, 0), adjoint, with_bias, 1) == k, (entry, adjoint, with_bias)
            k1 = ids(entry, 2, 30, 30, MASK.get(entry, 0), adjoint, with_bias, 1)
            assert k1 == [s.replace("<4, ", "<1, ").replace("blit_tile_kernel<", "blit_row_kernel<1, ").replace("tile", "px") for s in k] or entry == COLOR, (entry, k1)
    assert ids(COLOR, 1, 5, 7, 0, 1, 0, 1) == ["ada_color_px_kernel<true, false>"] and ids(COLOR, 1, 5, 7, 0, 0, 1, 1) == ["ada_color_px_kernel<false, true>"]


def rejected(L, code, words, entry, B, H, W, bits=0, adjoint=0, with_bias=0, aligned=1):
    L.sgx_clear_error()
    rc, out = AR.query(L, entry, B, H, W, bits, adjoint, with_bias, aligned)
    msg = L.sgx_last_error().decode(errors="replace")
    L.sgx_clear_error()
    assert rc == code and words in msg and out == [0] * AR.PLAN_INTS, (entry, B, H, W, bits, rc, msg, out)


def test_rejections(lib):
    for entry, name in enumerate(AR.ENTRY_NAME):
        for B in (0, 65536):
            rejected(lib, AR.EINVAL, f"{name}: bad arguments (B={B} 8x8)", entry, B, 8, 8)
        rejected(lib, AR.EINVAL, f"{name}: bad arguments", entry, 1, 0, 8)
        rejected(lib, AR.EINVAL, f"{name}: bad arguments", entry, 1, 8, -1)
        rejected(lib, AR.EUNSUPPORTED, f"{name}: image of 40000x40000 too large", entry, 1, 40000, 40000)
        assert AR.query(lib, entry, 65535, 8, 8)[0] == 0
    for entry, bad in ((DIFFAUG, (8, 16, 32, -1)), (GATED, (8, 16, 32, -1)), (BLIT, (32, 64, 256, -1))):
        for bits in bad:
            rejected(lib, AR.EINVAL, f"{AR.ENTRY_NAME[entry]}: policy bits {bits}", entry, 1, 8, 8, bits)
    for bits in (16, 31):
        rejected(lib, AR.EINVAL, "diffaug_blit: rot90 needs square images, got 8x12", BLIT, 1, 8, 12, bits)
    assert AR.query(lib, BLIT, 1, 8, 12, 15)[0] == 0          # xflip works for any H, W
    rejected(lib, AR.EINVAL, "ada_color: the adjoint has no bias", COLOR, 1, 8, 8, 0, 1, 1)
    for entry in (-1, 5):
        rejected(lib, AR.EINVAL, f"aug_plan: entry {entry}", entry, 1, 8, 8)
    lib.sgx_clear_error()
    assert lib.sgx_aug_plan(DIFFAUG, 1, 8, 8, 7, 0, 1, 1, None) == AR.EINVAL and b"out is NULL" in lib.sgx_last_error()
    lib.sgx_clear_error()


def test_workspace_is_the_partials_of_the_query(lib):
    for B, H, W in ((1, 4, 4), (3, 128, 128), (2, 128, 129), (2, 132, 132), (4, 1024, 1024), (7, 33, 20)):
        for entry in (DIFFAUG, GATED, BLIT):
            s = AR.lib_plan(lib, entry, B, H, W, 1)[0]
            assert lib.sgx_diffaug_ws_bytes(B, H, W) == 4 * B * s.nparts == 4 * B * s.gx, (B, H, W, s)
    assert AR.lib_plan(lib, DIFFAUG, 4, 1024, 1024, 1)[0].nparts == 64
    assert lib.sgx_diffaug_ws_bytes(0, 8, 8) == 0 and lib.sgx_diffaug_ws_bytes(1, 0, 8) == 0


def test_one_launch_site_per_kernel():
    """14 kernels, 14 hipLaunchKernelGGL sites over the three files; a 15th site fails."""
    sites = [s[0] for f in FILES for s in TSC.launch_sites(os.path.join(TSC.CSRC, f))]
    kernels = set()
    for f in FILES:
        with open(os.path.join(TSC.CSRC, f)) as fh:
            kernels |= set(re.findall(r"__global__\s+(?:__launch_bounds__\(\w+\)\s+)?void\s+([A-Za-z_0-9]+)", fh.read()))
    assert kernels == set(AR.KERNELS + AR.OTHER_KERNELS) and len(kernels) == 14, kernels ^ set(AR.KERNELS + AR.OTHER_KERNELS)
    assert len(sites) == 14 and collections.Counter(sites) == {k: 1 for k in kernels}, collections.Counter(sites)
    assert collections.Counter(sites + ["diffaug_apply_kernel"]) != {k: 1 for k in kernels}
