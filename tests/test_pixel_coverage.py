"""CPU side of tests/test_gpu_pixel_paths.py: (a) every launch site of csrc/diffaug.hip and every instantiation its dispatch lists can
reach (26 of the five image-pass kernels, the three controller kernels) is claimed by a row of pixel_ref.CASES, and a planted site or
a dropped row is noticed (the table is pinned: rows per entry and per shape, and a digest of the ids); (b) the kernels a row states are
what sgx_aug_plan answers for it; (c) the rows reach their seams, computed from the restated parameters; (d) the references alone have
the properties the GPU rows rely on and agree with diffaug_ref and blit_ref; (e) a numpy fp32 emulation of the kernels' own arithmetic
passes the criterion on every small row, the worst ratio printed; (f) nine kinds of planted error, in thirteen instances, fail it with
the element named -- and what the criterion that held these kernels before (1e-5 of the batch maximum) makes of the same tensors is
printed and pinned."""
import collections
import hashlib
import itertools
import os
import re

import numpy as np
import pytest
import torch

import aug_ref as AR
import blit_ref as Bl
import diffaug_ref as R
import pixel_ref as PR
import test_streaming_coverage as TSC
from pixel_ref import BLIT, DIFFAUG, GATED

DA = os.path.join(TSC.CSRC, "diffaug.hip")
f4, f8 = np.float32, np.float64
ENTRY = {DIFFAUG: AR.DIFFAUG, GATED: AR.GATED, BLIT: AR.BLIT}
NAMED = r"first at \(b, i, j, ch\) = "


@pytest.fixture(scope="module")
def lib():
    from stylegan.pytorch_amd import native
    native.build()
    return native.lib()


def source():
    with open(DA) as f:
        return f.read()


def find(entry, H, W, policy, mode, gated=False, variant=None):
    rows = [c for c in PR.IMAGE_CASES if c.entry == entry and (c.args["H"], c.args["W"], c.args["policy"]) == (H, W, policy) and
            (c.args["adjoint"], c.args["with_bias"]) == mode and bool(c.args["gated"]) == gated and (variant is None or c.args["variant"] == variant)]
    assert rows, (entry, H, W, policy, mode, gated)
    return rows[0]


# ---------------------------------------------------------------------------------------------------------------- (a) the scan
SITE = re.compile(r"hipLaunchKernelGGL\(\(?(\w+)(?:<([^;]*?)>\))?,")


def reachable(src):
    """Every instantiation the launch sites of the file can be given: a site's template arguments P(), M(), G() run through the
    sgx_by_int lists of da_by_targs (P and G in its body, M the list the site's case passes) or of the sgx_by_int around the site."""
    enum = dict(re.findall(r"\b(DA_[A-Z]+) = (\d+)", src))
    body = src[src.index("static void da_by_targs"):]
    body = body[:body.index("\n}")]
    assert "sgx_by_int<Ms...>(l.mode" in body
    Pv = [v.strip() for v in re.search(r"sgx_by_int<([^<>]*)>\(l\.P", body).group(1).split(",")]
    Gv = [v.strip() for v in re.search(r"sgx_by_int<([^<>]*)>\(l\.gated", body).group(1).split(",")]
    tf = lambda v: "true" if int(v) else "false"
    out = []
    for m in SITE.finditer(src):
        name, targs = m.groups()
        if not targs:
            out.append(name)
            continue
        window = src[max(src.rfind("case ", 0, m.start()), 0):m.start()]
        lists = re.findall(r"da_by_targs<([^<>]*)>\(l,", window) + re.findall(r"sgx_by_int<([^<>]*)>\(l\.mode", window)
        Mv = [enum.get(v.strip(), v.strip()) for v in lists[-1].split(",")] if lists else [None]
        args = [a.strip() for a in targs.split(",")]
        for P, M, G in itertools.product(Pv if "P()" in args else [None], Mv if any("M()" in a for a in args) else [None], Gv if any("G()" in a for a in args) else [None]):
            render = {"P()": P, "M()": M, "bool(M())": M and tf(M), "bool(G())": G and tf(G)}
            out.append(f"{name}<{', '.join(render.get(a, a) for a in args)}>")
    return out


def claimed(cases):
    return {k for c in cases for k in c.kernels}


def test_every_launch_site_and_instantiation_of_diffaug_hip_has_a_row():
    src = source()
    sites = TSC.launch_sites(DA)
    kernels = set(re.findall(r"__global__\s+(?:__launch_bounds__\(\w+\)\s+)?void\s+([A-Za-z_0-9]+)", src))
    assert kernels == set(PR.KERNELS) | set(PR.CONTROLLER.values()), kernels
    assert len(sites) == 8 and collections.Counter(s[0] for s in sites) == {k: 1 for k in kernels}, sites
    assert TSC.unclaimed(sites, PR.CASES, {}) == []
    reach = reachable(src)
    assert len(reach) == len(set(reach)) == PR.INSTANTIATIONS + 3, reach
    per = collections.Counter(k.split("<")[0] for k in reach)
    assert [per[k] for k in PR.KERNELS] == [8, 8, 4, 4, 2], per
    assert set(reach) == claimed(PR.CASES), set(reach) ^ claimed(PR.CASES)
    assert len({c.id for c in PR.CASES}) == len(PR.CASES) and all(c.why and c.kernels for c in PR.CASES)
    assert {c.entry for c in PR.CASES} == {DIFFAUG, GATED, BLIT} | set(PR.CONTROLLER)
    print(f"{len(PR.CASES)} rows, {len(PR.LARGE)} of them above 132 x 132")


# Rows per entry point and per (B, H, W, base offset), and a digest of the ids (an id spells entry, shape, offset, policy, mode, gated,
# draw layout and variant).  A row is a launch path someone decided to cover: dropping or changing one has to be a decision made here too.
ROWS = {DIFFAUG: 161, GATED: 266, BLIT: 556, "sgx_ada_gates": 1, "sgx_ada_gates_n": 1, "sgx_ada_update": 1}
ROWS_PER_SHAPE = {(3, 1, 1, 0): 24, (3, 1, 5, 0): 24, (3, 3, 2, 0): 24, (3, 2, 3, 0): 24, (8, 4, 4, 0): 135, (8, 5, 7, 0): 117, (8, 9, 12, 0): 117, (8, 6, 10, 0): 117,
                  (8, 16, 16, 1): 135, (5, 36, 36, 0): 24, (5, 17, 17, 0): 24, (2, 128, 128, 0): 24, (2, 128, 132, 0): 24, (2, 127, 131, 0): 24, (2, 132, 132, 0): 12,
                  (8, 8, 8, 0): 72, (8, 32, 32, 0): 18, (8, 36, 36, 0): 18, (8, 64, 64, 0): 18, (1, 1028, 1028, 0): 8}
IDS_SHA256 = "ca5224fca574609c2130e02bbc862bb3897f97d9ec3e6b31d061a125f455b2f7"


def table_is_pinned(cases):
    image = [c for c in cases if c.entry in (DIFFAUG, GATED, BLIT)]
    return (dict(collections.Counter(c.entry for c in cases)) == ROWS and
            dict(collections.Counter((c.args["B"], c.args["H"], c.args["W"], c.args["off"]) for c in image)) == ROWS_PER_SHAPE and
            hashlib.sha256("\n".join(c.id for c in cases).encode()).hexdigest() == IDS_SHA256)


def test_the_table_is_pinned_row_by_row():
    assert dict(collections.Counter(c.entry for c in PR.CASES)) == ROWS
    assert dict(collections.Counter((c.args["B"], c.args["H"], c.args["W"], c.args["off"]) for c in PR.IMAGE_CASES)) == ROWS_PER_SHAPE
    assert table_is_pinned(PR.CASES) and len(PR.CASES) == 986
    for c in PR.CASES:                                       # an id says what the row is
        a = c.args
        if c.entry in PR.CONTROLLER:
            assert c.id == f"{c.entry[4:]}-B{a['B']}"
            continue
        want = (f"{c.entry[4:]}-B{a['B']}-{a['H']}x{a['W']}{'+%d' % a['off'] if a['off'] else ''}-p{a['policy']}-{PR.MODE_NAME[(a['adjoint'], a['with_bias'])]}"
                f"{'-gated' if a['gated'] else ''}{'-wide' if a['wide'] else ''}{'-v1' if a['variant'] else ''}")
        assert c.id == want and c.kernels == PR.kernels_of(c.entry, a["H"], a["W"], a["off"], a["policy"], a["adjoint"]), c.id
    for k in (0, 1, len(PR.CASES) // 2, len(PR.CASES) - 4, len(PR.CASES) - 1):               # any one row removed is noticed
        assert not table_is_pinned(PR.CASES[:k] + PR.CASES[k + 1:]), PR.CASES[k].id
    assert not table_is_pinned([c for c in PR.CASES if c.id != "diffaug-B8-4x4-p3-lin"])


def test_a_new_site_or_a_dropped_row_is_noticed():
    src = source()
    base = set(reachable(src))
    for extra, new in (("hipLaunchKernelGGL((diffaug_apply_kernel<8, true, false>), grid, block", {"diffaug_apply_kernel<8, true, false>"}),
                       ("hipLaunchKernelGGL(diffaug_blit_col_kernel, grid, block", {"diffaug_blit_col_kernel"})):
        assert set(reachable(src + "\n" + extra)) - claimed(PR.CASES) == new
    wider = src.replace("sgx_by_int<1, 4>(l.P", "sgx_by_int<1, 2, 4>(l.P")
    assert wider != src and len(set(reachable(wider)) - claimed(PR.CASES)) == 12
    third = src.replace("da_by_targs<DA_PLAIN, DA_ADJ>(l, [&](auto P, auto M, auto G)", "da_by_targs<DA_PLAIN, DA_FWD, DA_ADJ>(l, [&](auto P, auto M, auto G)")
    assert third != src and set(reachable(third)) - claimed(PR.CASES) == {f"diffaug_sum_kernel<{P}, 1, {g}>" for P in (1, 4) for g in ("true", "false")}
    assert TSC.unclaimed(TSC.launch_sites(DA) + [("diffaug_blit_col_kernel", "")], PR.CASES, {}) == ["diffaug_blit_col_kernel"]
    for k in sorted(base):                                   # every instantiation: without the rows that name it, it is missed
        missed = base - claimed([c for c in PR.CASES if k not in c.kernels])         # (a sum pass runs with one apply kernel only: those rows take it along)
        assert k in missed and {m.split("<")[0] for m in missed} <= {k.split("<")[0], "diffaug_sum_kernel", "diffaug_blit_sum_kernel"}, (k, missed)
    assert len(PR.LARGE) == 8 and [c.args["B"] for c in PR.LARGE] == [1] * 8 and all((c.args["H"], c.args["W"]) == (1028, 1028) for c in PR.LARGE)
    assert max(max(c.args["H"], c.args["W"]) for c in PR.IMAGE_CASES if c not in PR.LARGE) == 132


# ---------------------------------------------------------------------------------------------------------------- (b) the plan
def test_the_kernels_of_every_row_are_what_the_plan_query_answers(lib):
    for c in PR.IMAGE_CASES:
        a = c.args
        got = AR.launches_of(AR.lib_plan(lib, ENTRY[c.entry], a["B"], a["H"], a["W"], a["policy"], a["adjoint"], a["with_bias"], int(a["off"] == 0)))[0]
        assert tuple(got) == c.kernels, (c.id, got, c.kernels)
        assert lib.sgx_diffaug_ws_bytes(a["B"], a["H"], a["W"]) == 4 * a["B"] * PR.nparts(a["H"], a["W"])


# ---------------------------------------------------------------------------------------------------------------- (c) the seams
def group_branches(p, H, W, adjoint):
    """da_load<4> restated on whole groups: -> (groups taking the three 16-byte loads, groups going pixel by pixel)."""
    i, j0 = np.mgrid[0:H, 0:W:4]
    si, sj0 = (i - p["tx"], j0 - p["ty"]) if adjoint else (i + p["tx"], j0 + p["ty"])
    mi, mj0 = (si, sj0) if adjoint else (i, j0)
    row_cut = (mi >= p["r0"]) & (mi < p["r1"])
    none_cut = ~row_cut | (mj0 + 4 <= p["c0"]) | (mj0 >= p["c1"])
    fast = (si >= 0) & (si < H) & (sj0 >= 0) & (sj0 + 4 <= W) & none_cut
    return int(fast.sum()), int((~fast).sum())


def row_params(c):
    a = c.args
    _, u = PR.inputs(c)
    return [PR.params_of(u[n], a["H"], a["W"], b) for n, b in enumerate(PR.effective_bits(c))], u


def test_rows_reach_their_seams():
    rows = PR.IMAGE_CASES
    by_shape = collections.defaultdict(list)
    for c in rows:
        by_shape[(c.args["B"], c.args["H"], c.args["W"], c.args["off"])].append(c)
    # the shapes the issue lists, and on each what it asks
    assert set(by_shape) == {(3, 1, 1, 0), (3, 1, 5, 0), (3, 3, 2, 0), (3, 2, 3, 0), (8, 4, 4, 0), (8, 5, 7, 0), (8, 9, 12, 0), (8, 6, 10, 0), (8, 16, 16, 1), (5, 36, 36, 0),
                             (5, 17, 17, 0), (2, 128, 128, 0), (2, 128, 132, 0), (2, 127, 131, 0), (2, 132, 132, 0), (1, 1028, 1028, 0), (8, 8, 8, 0), (8, 32, 32, 0), (8, 36, 36, 0),
                             (8, 64, 64, 0)}
    for shape, cs in by_shape.items():
        B, H, W, off = shape
        entries = {c.entry for c in cs}
        modes = {(c.args["adjoint"], c.args["with_bias"]) for c in cs}
        assert modes == (set(PR.MODES) if H <= 132 else {(0, 1), (1, 0)}), shape
        assert any(c.args["policy"] & 1 for c in cs) and any(not c.args["policy"] & 1 for c in cs) or H > 132, shape
        if shape[:3] in ((8, 4, 4), (8, 5, 7), (8, 9, 12), (8, 6, 10), (8, 16, 16)):
            assert entries == {DIFFAUG, GATED, BLIT}
            for e in (DIFFAUG, GATED):
                assert {c.args["policy"] for c in cs if c.entry == e} == set(range(1, 8)), shape
            assert {c.args["policy"] for c in cs if c.entry == BLIT} == set(PR.SQUARE if H == W else PR.FLAT), shape
        if entries >= {BLIT}:
            bl = [c for c in cs if c.entry == BLIT]
            assert {bool(c.args["gated"]) for c in bl} == ({False, True} if H <= 132 else {False}) and ({c.args["wide"] for c in bl} == {0, 1} or H > 132), shape
        if H < 4 or W < 4:
            assert entries == {DIFFAUG, GATED, BLIT} and all(bool(c.args["policy"] & 16) == (H == W) for c in cs if c.entry == BLIT), shape
    assert {c.args["policy"] for c in rows if c.entry == BLIT and c.args["H"] == 8} == set(PR.SQUARE)
    # gated batches hold every bit pattern, 0 among them
    for variant in (0, 1):
        assert sorted(PR.gates_of(GATED, 8, 7, variant)) == list(range(8)) and all(0 in PR.gates_of(e, B, 31 if e == BLIT else 7, variant) for e in (GATED, BLIT) for B in (3, 5, 8))
        assert {b & 24 for b in PR.gates_of(BLIT, 8, 31, variant)} == {0, 8, 16, 24}
    # what each entry's rows carry on the single-block shapes, under the bits the images have: a row of draws that is 0.0 in every column
    # with every op on, one that is 1.0 in every column with the two ops that draw an integer on, and the cutout's first and last column on
    # every residue mod 4 with the box inside the row
    for shape in ((8, 4, 4, 0), (8, 5, 7, 0), (8, 9, 12, 0), (8, 6, 10, 0), (8, 16, 16, 1)):
        for entry in (DIFFAUG, GATED, BLIT):
            zeros, ones, c0s, c1s = False, False, set(), set()
            for c in by_shape[shape]:
                if c.entry != entry:
                    continue
                ps, u = row_params(c)
                for n, (p, b) in enumerate(zip(ps, PR.effective_bits(c))):
                    zeros |= bool((u[n] == 0.0).all()) and b & 7 == 7
                    ones |= bool((u[n] == 1.0).all()) and b & 6 == 6
                    if b & 4 and p["c1"] - p["c0"] == (shape[2] + 1) // 2:
                        c0s.add(p["c0"] % 4); c1s.add(p["c1"] % 4)
            full = {0, 1, 2, 3} if shape[2] > 4 else {0, 1, 2}                     # (W = 4, cw = 2: a box from column 3 is clipped)
            assert zeros and ones and c0s == full and c1s == {(r + (shape[2] + 1) // 2) % 4 for r in full}, (shape, entry, zeros, ones, c0s, c1s)
    # nparts, units, the large rows
    assert {PR.nparts(c.args["H"], c.args["W"]) for c in rows if c.args["policy"] & 1} == {1, 2, 65}
    assert PR.nparts(128, 128) == 1 and PR.nparts(128, 132) == PR.nparts(127, 131) == PR.nparts(132, 132) == 2 and PR.nparts(1028, 1028) == 65 and PR.nparts(1024, 1024) == 64
    assert [PR.n_M(4, 1), PR.n_M(1, 2), PR.n_M(4, 65)] == [46, 85, 47]
    assert 256 < 36 * 36 // 4 == 324 <= 512 and 256 < 17 * 17 == 289 <= 512 and PR.pixels_per_lane(36, 0) == 4 and PR.pixels_per_lane(17, 0) == 1
    assert {(c.entry, c.args["policy"], c.args["adjoint"]) for c in PR.LARGE} == {(e, p, a) for e, p in ((DIFFAUG, 7), (GATED, 7), (BLIT, 31), (BLIT, 15)) for a in (0, 1)}
    # draws: u exactly 0.0 and 1.0 in every column, 1.0 clamped in every draw; translations at +-sh, +-sw
    for (B, H, W, off) in by_shape:
        for variant in (0, 1):
            u = PR.draws(B, H, W, variant, seed=H + W)
            assert u.dtype == f4 and u.shape == (B, 9) and float(u.min()) >= 0.0 and float(u.max()) <= 1.0
            for n in range(B):                               # b and c are the kernels' fp32 numbers, and 1 - c is exact in fp32
                p = PR.params_of(u[n], H, W, 1)
                assert p["b"] == float(f4(u[n, 0]) - f4(0.5)) and p["c"] == float(f4(u[n, 2]) + f4(0.5)) and float(f4(1) - f4(p["c"])) == 1.0 - p["c"]
            sh, sw = (H + 4) // 8, (W + 4) // 8
            ps = [PR.params_of(u[n], H, W, 31 if H == W else 15) for n in range(B)]
            assert all(abs(p["tx"]) == sh and abs(p["ty"]) == sw for p in ps), (B, H, W)
            if B > 1 and not variant:
                assert bool((u == 1.0).all(axis=1).any()), (B, H, W)
            if B >= 3 and not variant:
                assert bool((u == 0.0).all(axis=1).any()), (B, H, W)
            if B == 8:
                assert {(p["tx"] > 0, p["ty"] > 0) for p in ps} == set(itertools.product((False, True), repeat=2)) or sh == 0 or sw == 0
                assert {(p["f"], p["k"]) for p in ps} == set(itertools.product((0, 1), range(4))) or H != W
        ch, cw = (H + 1) // 2, (W + 1) // 2
        for n_, hi in ((2 * sh + 1, 2 * sh), (2 * sw + 1, 2 * sw), (H + 1 - ch % 2, H - ch % 2), (W + 1 - cw % 2, W - cw % 2), (2, 1), (4, 3)):
            assert int(np.floor(f4(1.0) * f4(n_))) == hi + 1 and R._draw(1.0, n_, hi) == hi          # u = 1.0: the clamp decides
    # below 4: no shift on that side; the cutout one row / column or the whole image; W = 1
    for H, W in ((1, 1), (1, 5), (3, 2), (2, 3)):
        ps = [PR.params_of(PR.draws(3, H, W, v, seed=H + W)[n], H, W, 7) for v in (0, 1) for n in range(3)]
        assert all((H >= 4 or p["tx"] == 0) and (W >= 4 or p["ty"] == 0) for p in ps)
        assert {p["r1"] - p["r0"] for p in ps} <= {0, 1, 2} and any(p["r1"] - p["r0"] == min(H, (H + 1) // 2) for p in ps)
    assert any((p["r0"], p["r1"], p["c0"], p["c1"]) == (0, 1, 0, 1) for p in [PR.params_of(PR.draws(3, 1, 1, 0, seed=2)[n], 1, 1, 7) for n in range(3)])
    # both branches of da_load and da_load_blit at every residue of the cutout's edges, the box inside a row of groups
    for B, H, W, off in ((8, 9, 12, 0), (8, 8, 8, 0), (8, 32, 32, 0), (8, 36, 36, 0), (8, 64, 64, 0)):
        seen = collections.defaultdict(set)
        for variant, adjoint in itertools.product((0, 1), (0, 1)):
            u = PR.draws(B, H, W, variant, seed=H + W)
            for n in range(B):
                p = PR.params_of(u[n], H, W, 7)
                fast, slow = group_branches(p, H, W, adjoint)
                if p["c1"] - p["c0"] == (W + 1) // 2 and fast and slow:
                    seen["c0"].add(p["c0"] % 4); seen["c1"].add(p["c1"] % 4)
        assert seen["c0"] == seen["c1"] == {0, 1, 2, 3}, (H, W, dict(seen))
    both = [group_branches(p, c.args["H"], c.args["W"], c.args["adjoint"]) for c in rows if c.kernels[-1].startswith(("diffaug_apply_kernel<4", "diffaug_blit_row_kernel<4")) and c.args["policy"] & 6 and c.args["H"] >= 4
            for p in row_params(c)[0][:1]]
    assert both and all(f + s > 0 for f, s in both) and any(f for f, _ in both) and any(s for _, s in both)
    # the tile kernel: N = 4, 8, 32, 36, 64; on the tiles without overhang the source square of a border tile leaves the image on each of the
    # four sides under each of the eight orientations, forward and inverse
    tile_rows = [c for c in rows if c.kernels[-1].startswith("diffaug_blit_tile_kernel") and c.args["H"] <= 132]
    assert {c.args["H"] for c in tile_rows} == {4, 8, 32, 36, 64, 132} and all(c.args["B"] == 8 for c in tile_rows if c.args["H"] <= 64)
    for N in (32, 64):
        for adjoint in (0, 1):
            left = set()
            for c in tile_rows:
                if c.args["H"] != N or c.args["adjoint"] != adjoint or c.args["gated"]:
                    continue
                for p in row_params(c)[0]:
                    si, sj, _ = PR.index_map(p, N, N, adjoint)
                    for I0, J0 in itertools.product(range(0, N, 32), repeat=2):
                        r0, c0 = min(si[I0, J0], si[I0 + 31, J0 + 31]), min(sj[I0, J0], sj[I0 + 31, J0 + 31])
                        assert abs(int(si[I0, J0]) - int(si[I0 + 31, J0 + 31])) == 31 == abs(int(sj[I0, J0]) - int(sj[I0 + 31, J0 + 31]))
                        left |= {(p["f"], p["k"], side) for side, out in (("top", r0 < 0), ("bottom", r0 + 32 > N), ("left", c0 < 0), ("right", c0 + 32 > N)) if out}
            assert len(left) == 32, (N, adjoint, sorted(left))
    # all eight orientations, forward and inverse, on the tile kernel and on both row kernels
    for head in ("diffaug_blit_tile_kernel", "diffaug_blit_row_kernel<1", "diffaug_blit_row_kernel<4"):
        for adjoint in (0, 1):
            got = {(p["f"], p["k"]) for c in rows if c.kernels[-1].startswith(head) and c.args["adjoint"] == adjoint for p in row_params(c)[0]}
            assert got == set(itertools.product((0, 1), range(4) if "<4" not in head else (0,))), (head, adjoint, got)


# ---------------------------------------------------------------------------------------------------------------- (d) the references alone
def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2)


def test_references_alone_have_what_the_gpu_rows_rely_on():
    checked = 0
    for c in PR.IMAGE_CASES:
        a = c.args
        if a["H"] > 36 or (a["wide"] and not a["gated"]):
            continue
        x, u = PR.inputs(c)
        bits = PR.effective_bits(c)
        ref, exact, bound = PR.expected(c, x, u)
        # the structured restatement of blit_ref (diffaug_ref's ops with torch.flip / torch.rot90), image by image, on the same parameters
        x64 = nchw(x.astype(f8))
        want = torch.stack([Bl.apply_one(x64[n], PR.params_of(u[n], a["H"], a["W"], b), b, bool(a["adjoint"]), bool(a["with_bias"])) for n, b in enumerate(bits)]).permute(0, 2, 3, 1).numpy()
        scale = np.abs(want).max(axis=(1, 2, 3), keepdims=True) + np.abs(x.astype(f8)).max(axis=(1, 2, 3), keepdims=True)
        assert bool((np.abs(ref - want) <= 1e-13 * scale).all()), c.id
        for n, b in enumerate(bits):
            p = PR.params_of(u[n], a["H"], a["W"], b)
            _, _, ok = PR.index_map(p, a["H"], a["W"], a["adjoint"])
            if not b & 1:
                assert bool(exact[n].all()) and not bound[n].any() and np.array_equal(ref[n].astype(f4).view(np.int32), np.where(ok[..., None], ref[n], 0.0).astype(f4).view(np.int32))
                assert not np.signbit(ref[n][~ok]).any()
            elif a["adjoint"]:
                assert not exact[n].any() and (bool((bound[n] > 0).all()) or a["H"] * a["W"] < 16)
            else:
                assert np.array_equal(exact[n], np.broadcast_to(~ok[..., None], exact[n].shape)) and not ref[n][exact[n]].any() and not np.signbit(ref[n][exact[n]]).any()
                assert bool((bound[n][~exact[n]] > 0).all()) or a["H"] * a["W"] < 16
        checked += 1
    assert checked > 300
    # the index rules against blit_ref.literal (pixel by pixel) and the colour against diffaug_ref.literal (DiffAugment's published indexing)
    for H, W, policy in ((8, 8, 30), (4, 4, 30), (5, 7, 14), (1, 5, 14), (3, 2, 14), (1, 1, 30)):
        x = PR.images(8, H, W, 5, False).astype(f8)
        for variant, adjoint in itertools.product((0, 1), (0, 1)):
            u = PR.draws(8, H, W, variant, seed=3)
            ref, _, _ = PR.reference(x, u, [policy] * 8, adjoint, 0, 1)
            for n in range(8):
                lit = Bl.literal(nchw(x[n:n + 1])[0], PR.params_of(u[n], H, W, policy), bool(adjoint)).permute(1, 2, 0).numpy()
                assert np.array_equal(ref[n], lit), (H, W, variant, adjoint, n)
    for H, W in ((8, 8), (5, 7), (9, 12)):
        x = PR.images(8, H, W, 6).astype(f8)
        u = PR.draws(8, H, W, 0, seed=4)
        ref, _, _ = PR.reference(x, u, [7] * 8, 0, 1, 1)
        ch, cw = (H + 1) // 2, (W + 1) // 2
        for n in range(8):
            p, q = PR.params_of(u[n], H, W, 7), R.params(u[n, :7], H, W, 7)
            assert all(p[k] == q[k] for k in ("s", "tx", "ty", "r0", "r1", "c0", "c1")) and abs(p["b"] - q["b"]) <= PR.U and abs(p["c"] - q["c"]) <= PR.U
            p.update(ox=R._draw(u[n, 5], H + 1 - ch % 2, H - ch % 2), oy=R._draw(u[n, 6], W + 1 - cw % 2, W - cw % 2))
            lit = R.literal(nchw(x[n:n + 1]), p, 7).permute(0, 2, 3, 1).numpy()[0]
            assert float(np.abs(ref[n] - lit).max()) <= 1e-13 * float(np.abs(lit).max()), (H, W, n)
    # the adjoint identity in fp64: <A x, g> = <x, A^T g> with A the linear part
    for c in PR.IMAGE_CASES:
        a = c.args
        if (a["adjoint"], a["with_bias"]) != (0, 0) or a["H"] > 36:
            continue
        x, u = PR.inputs(c)
        g = PR.images(a["B"], a["H"], a["W"], 77).astype(f8)
        bits, P = PR.effective_bits(c), PR.pixels_per_lane(a["W"], a["off"])
        ax = PR.reference(x.astype(f8), u, bits, 0, 0, P)[0]
        atg = PR.reference(g, u, bits, 1, 0, P)[0]
        lhs, rhs = (ax * g).sum(axis=(1, 2, 3)), (x.astype(f8) * atg).sum(axis=(1, 2, 3))
        assert bool((np.abs(lhs - rhs) <= 1e-12 * (np.abs(ax * g).sum(axis=(1, 2, 3)) + np.abs(x * atg).sum(axis=(1, 2, 3)))).all()), c.id
    # inputs of colour rows: a mean of the order of the spread, amplitudes from 1e-3 to 1e3 within a batch
    for B in (2, 3, 5, 8):
        x = PR.images(B, 8, 8, 1).astype(f8)
        amp, mean = x.std(axis=(1, 2, 3)), np.abs(x.mean(axis=(1, 2, 3)))
        assert amp.min() < 2e-3 and amp.max() > 5e2 and bool((mean > 0.3 * amp).all()) and len(set(np.round(mean / amp, 1))) >= 2


# ---------------------------------------------------------------------------------------------------------------- (e) the emulation
LANES = np.arange(64)


def butterfly(a):
    """wave_sum: six steps of v += shfl_xor(v, o), o = 32 .. 1, on the last axis (64 lanes)."""
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., LANES ^ o]
    return a


def emu_partials(src, P):
    """diffaug_sum_kernel / diffaug_blit_sum_kernel on one image, fp32 [H][W][3] -> the partials: a unit's 3P values added in order,
    a thread's UPT units in order, wave_sum, the four waves in order."""
    H, W, _ = src.shape
    un = src.reshape(-1, 3 * P)
    s = np.zeros(len(un), f4)
    for k in range(3 * P):
        s = s + un[:, k]
    parts, upt = PR.nparts(H, W), PR.PART_PIXELS // (PR.BLOCK * P)
    full = np.zeros(parts * upt * PR.BLOCK, f4)
    full[:len(s)] = s
    full = full.reshape(parts, upt, PR.BLOCK)
    acc = np.zeros((parts, PR.BLOCK), f4)
    for it in range(upt):
        acc = acc + full[:, it]
    w = butterfly(acc.reshape(parts, 4, 64))[..., 0]
    t = w[:, 0]
    for k in range(1, 4):
        t = t + w[:, k]
    return t


def emu_mean(part, H, W, over_hw=False):
    """The finishing loop: lane l adds partials l, l + 64, ... in order, wave_sum, the quotient by 3 H W."""
    t = np.zeros(64, f4)
    for k0 in range(0, len(part), 64):
        chunk = np.zeros(64, f4)
        chunk[:len(part[k0:k0 + 64])] = part[k0:k0 + 64]
        t = t + chunk
    return butterfly(t)[0] / ((f4(1) if over_hw else f4(3)) * f4(H) * f4(W))


def emulate(x, u, bits, adjoint, with_bias, P, plant=None):
    """The launch in numpy fp32, every operation rounded on its own in the kernels' order (no fma).  ``plant``: one of the errors of (f)."""
    B, H, W, _ = x.shape
    y, maps, parts = np.zeros_like(x), [], []
    for n in range(B):
        p = PR.params_of(u[n], H, W, bits[n])
        if plant == "r1" and bits[n] & 4:
            p["r1"] = min(p["r1"] + 1, H)
        si, sj, ok = PR.index_map(p, H, W, adjoint, cut_at_output=plant == "cut_at_output")
        v = PR.gather(x[n], si, sj, ok)
        if plant == "not_reversed" and p["f"] and not p["k"] & 1 and P == 4:
            v4, whole = v.reshape(H, W // 4, 4, 3).copy(), ok.reshape(H, W // 4, 4).all(-1)
            v4[whole] = v4[whole][:, ::-1]
            v = v4.reshape(H, W, 3)
        maps.append((p, ok, v))
        parts.append(emu_partials(v if adjoint else x[n], P) if bits[n] & 1 else None)
    for n in range(B):
        p, ok, v = maps[n]
        if not bits[n] & 1:
            y[n] = v
            continue
        part = parts[n]
        if plant == "neighbour":
            part = next(parts[(n + k) % B] for k in range(1, B + 1) if parts[(n + k) % B] is not None)
        if plant == "drop_last":
            part = part.copy()
            part[-1] = 0
        M = emu_mean(part, H, W, over_hw=plant == "M_over_HW")
        c, s, b = f4(u[n, 2]) + f4(0.5), f4(2) * f4(u[n, 1]), f4(u[n, 0]) - f4(0.5)
        biased = (with_bias or plant == "bias_in_linear") and not adjoint
        cs, k0 = c * s, (f4(1) - c) * M + (b if biased else f4(0))
        m = ((v[..., 0] + v[..., 1]) + v[..., 2]) * f4(1.0 / 3.0)
        cm = c * m + k0
        o = cs * (v - m[..., None]) + cm[..., None]
        y[n] = o if adjoint or plant == "mask_first" else np.where(ok[..., None], o, f4(0))
    if plant == "copy_small":
        n = int(np.argmin(PR.amplitudes(x)))
        y[n] = x[n]
    return y


def run_emulated(c, plant=None, x=None):
    a = c.args
    x0, u = PR.inputs(c)
    x = x0 if x is None else x
    bits, P = PR.effective_bits(c), PR.pixels_per_lane(a["W"], a["off"])
    y = emulate(x, u, bits, a["adjoint"], a["with_bias"], P, plant)
    return y, PR.reference(x.astype(f8), u, bits, a["adjoint"], a["with_bias"], P)


def test_the_emulation_passes_the_criterion_on_every_small_row():
    worst, done = collections.defaultdict(float), {}
    for c in PR.IMAGE_CASES:
        a = c.args
        if c in PR.LARGE:
            continue
        key = (a["B"], a["H"], a["W"], a["off"], a["policy"], a["adjoint"], a["with_bias"], tuple(PR.effective_bits(c)), a["variant"])
        if key not in done:
            y, (ref, exact, bound) = run_emulated(c)
            done[key] = PR.check(y, ref, exact, bound, "emulated " + c.id)
        worst[c.entry] = max(worst[c.entry], done[key])
    print("emulation, worst err / bound per entry over the small rows: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert all(0.0 < v <= 1.0 for v in worst.values()) and set(worst) == {DIFFAUG, GATED, BLIT}, dict(worst)


def test_the_emulation_passes_the_criterion_at_65_partials():
    c = find(BLIT, 1028, 1028, 15, (0, 1))
    y, (ref, exact, bound) = run_emulated(c)
    r = PR.check(y, ref, exact, bound, "emulated " + c.id)
    print(f"emulation, {c.id}: worst err / bound {r:.3f}")
    assert 0.0 < r <= 1.0


# ---------------------------------------------------------------------------------------------------------------- (f) planted errors
def planted(name, c, plant, where, old, x=None):
    y, (ref, exact, bound) = run_emulated(c, plant, x)
    err, tol, ok = PR.old_criterion(y, ref)
    print(f"planted {name} on {c.id}: max|y - ref| {err:.3e} against 1e-5 max|ref| = {tol:.3e}: the older criterion {'passes it' if ok else 'fails it'}")
    old[name] = ok
    with pytest.raises(AssertionError, match=NAMED + where):
        PR.check(y, ref, exact, bound, name)


def test_the_criterion_fails_the_planted_errors_with_the_element_named():
    old = {}
    two = find(DIFFAUG, 128, 132, 7, (0, 1))                 # two partials, two images: amplitudes 1e-3 and 1e3
    small = find(DIFFAUG, 9, 12, 7, (0, 1))
    honest, (ref, exact, bound) = run_emulated(two)
    assert PR.check(honest, ref, exact, bound, "honest") <= 1.0 and PR.old_criterion(honest, ref)[2]
    planted("a dropped last partial", two, "drop_last", r"\(0, 16, 17, 0\)", old)
    planted("partials of the neighbouring image", two, "neighbour", r"\(0, 16, 17, 0\)", old)
    planted("M over HW instead of 3HW", two, "M_over_HW", r"\(0, 16, 17, 0\)", old)
    planted("the bias present in the linear mode", find(DIFFAUG, 128, 132, 7, (0, 0)), "bias_in_linear", r"\(0, \d+, \d+, \d\)", old)
    planted("the forward mask applied before the colour", small, "mask_first", r"\(\d, \d+, \d+, \d\)", old)
    planted("the adjoint cutout tested at the output", find(DIFFAUG, 9, 12, 7, (1, 0)), "cut_at_output", r"\(\d, \d+, \d+, \d\)", old)
    planted("r1 off by one", small, "r1", r"\(\d, \d+, \d+, \d\)", old)
    planted("r1 off by one, no colour", find(DIFFAUG, 9, 12, 6, (0, 1)), "r1", r"\(\d, \d+, \d+, \d\)", old)
    planted("a flipped group not reversed", find(BLIT, 9, 12, 15, (0, 1)), "not_reversed", r"\(1, \d+, \d+, \d\)", old)
    planted("a flipped group not reversed, no colour", find(BLIT, 9, 12, 14, (0, 1)), "not_reversed", r"\(1, \d+, \d+, \d\)", old)
    planted("a small-amplitude image returned as a copy", find(DIFFAUG, 9, 12, 7, (0, 0)), "copy_small", r"\(0, \d+, \d+, \d\)", old)
    planted("a small-amplitude image returned as a copy, no colour", find(DIFFAUG, 9, 12, 6, (0, 1)), "copy_small", r"\(\d, \d+, \d+, \d\)", old)
    # the inputs of the older tests: zero-mean randn, where M is about 1 / sqrt(3 H W) and an error of the sum pass hides under the tolerance
    big = find(DIFFAUG, 1028, 1028, 7, (0, 1))
    planted("a dropped last partial, zero-mean data at 65 partials", big, "drop_last", r"\(0, \d+, \d+, \d\)", old, x=PR.images(1, 1028, 1028, 9, colour=False))
    # an unwritten element (the NaN prefill) fails both kinds of check
    nan = np.full((1, 1, 1, 3), np.nan, f4)
    one = np.ones((1, 1, 1, 3))
    for exact_ in (True, False):
        with pytest.raises(AssertionError, match=NAMED + r"\(0, 0, 0, 0\)"):
            PR.check(nan, one, np.full(one.shape, exact_), 1e30 * one, "sentinel")
    with pytest.raises(AssertionError, match="exact elements differ in bits"):
        PR.check(np.full((1, 1, 1, 3), -0.0, f4), np.zeros((1, 1, 1, 3)), np.ones((1, 1, 1, 3), bool), one, "sign of a masked zero")
    assert old == OLD, old


# what the older criterion (one number for the batch) makes of the planted errors above
OLD = {"a dropped last partial": False, "partials of the neighbouring image": False, "M over HW instead of 3HW": False, "the bias present in the linear mode": False,
       "the forward mask applied before the colour": False, "the adjoint cutout tested at the output": False, "r1 off by one": False, "r1 off by one, no colour": False,
       "a flipped group not reversed": False, "a flipped group not reversed, no colour": False,
       # the two it could not see: an image 10^6 times smaller than its neighbour, and the sum pass on the zero-mean inputs it was given
       "a small-amplitude image returned as a copy": True, "a small-amplitude image returned as a copy, no colour": False,
       "a dropped last partial, zero-mean data at 65 partials": True}
