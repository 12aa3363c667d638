"""CPU: what a call of the discriminator's composed first layer (sgx_rgbconv_pack / _fwd / _dgrad / _wgrad) will launch, asked of the library
itself.  sgx_rgbconv_plan answers from rgbconv_plan, the function the four entry points of csrc/rgbconv.hip execute, so on a grid of shapes with
points on both sides of every seam -- strips of 14 columns that do and do not divide the width, the row-block heuristic's steps at 1024^2,
every sgx_rgbconv_tune override, the three forward variants and the plain convolution, more tiles than three blocks per CU -- (a) kernel,
template arguments, grid, LDS and geometry arguments are what tests/rgbconv_ref.py restates; (b) sgx_rgbconv_wgrad_ws_bytes is the block count
of the query; (c) the persistent grid of rgbconv_fwd_kernel is ceil8(min(tiles, per_cu * CUs)) of the per_cu the query reports; (d) every row
of rgbconv_ref.CASES gets its kernel list and launch geometry from the query; (e) the shapes sgx_rgbconv_ok refuses, an unknown entry and a
NULL out are rejected.  The query is host-only: nothing here launches.  sgx_rgbconv_tune's state is process-wide: every test leaves
(-1, 0, 0) behind."""
import ctypes

import pytest
import torch

import rgbconv_ref as RR

PLAN_INTS = 11
PACK, FWD, DGRAD, WGRAD = 0, 1, 2, 3                         # SGX_RGBCONV_PLAN_*
ENTRY = {"sgx_rgbconv_pack": PACK, "sgx_rgbconv_fwd": FWD, "sgx_rgbconv_dgrad": DGRAD, "sgx_rgbconv_wgrad": WGRAD}
K_PACK, K_FWD, K_FWDBLUR, K_DGRAD, K_WGRAD = range(5)        # out[0]
HS, WS, BS = (16, 32, 48, 1024), (64, 128, 192, 448, 1024), (1, 2, 5)      # 448 = 32 strips of 14: the one width here without a ragged last strip
REFUSED = ((1, 8, 64, 16), (1, 16, 32, 16), (1, 24, 64, 16), (1, 16, 96, 16), (1, 16, 64, 24), (0, 16, 64, 16))


@pytest.fixture(scope="module")
def lib():
    from stylegan.pytorch_amd import native
    native.build()
    return native.lib()


@pytest.fixture(autouse=True)
def _tune_restored(lib):
    yield
    assert lib.sgx_rgbconv_tune(-1, 0, 0) == 0


def device_ncu():
    """The CU count sgx_ncu answers: the device's where there is one, 256 without."""
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else RR.NCU_NOMINAL


def lib_plan(L, entry, B, H, W, C, epi=0):
    out = (ctypes.c_int * PLAN_INTS)()
    rc = L.sgx_rgbconv_plan(entry, B, H, W, C, epi, ctypes.addressof(out))
    assert rc == 0, (entry, B, H, W, C, epi, rc, L.sgx_last_error())
    return list(out)


def launches_of(q):
    """The ints of the query as (kernel names in launch order, [(grid, block, dynamic LDS)]): the form of rgbconv_ref.plan and of the
    profiler's records (tests/test_gpu_rgbconv_paths.py)."""
    kind, CB, epi, grid, lds = q[:5]
    first = ((grid, 1, 1), RR.BLOCK, lds)
    if kind == K_WGRAD:
        return (f"rgbconv_wgrad_kernel<{CB}>", RR.WFINISH, RR.CHAIN), [first, ((q[8], 1, 1), RR.BLOCK, 0), ((q[9], 1, 1), RR.BLOCK, 0)]
    name = {K_PACK: RR.PACK, K_FWD: RR.fwd_kernel(CB, epi), K_FWDBLUR: RR.fwdblur_kernel(CB), K_DGRAD: f"rgbconv_dgrad_kernel<{CB}>"}[kind]
    return (name,), [first]


def persistent_fwd(q, B, H, W, CB, epi, ncu):
    """rgbconv_fwd_kernel<CB, epi> on a persistent grid: everything restated but the occupancy figure, which is held to its range and the
    grid to it."""
    g = RR.rc_fwd(CB, epi)
    nt = RR.fwd_ntiles(B, H, W, CB, epi)
    assert 1 <= q[10] <= 4, q
    assert q == [K_FWD, CB, epi, RR.ceil8(min(nt, q[10] * ncu)), g.LDS, W // g.TW, H // g.TH, nt, 0, 0, q[10]], (B, H, W, CB, epi, q)
    RR.check_rc_grid(q[3], nt, ncu, per_cu=q[10])


def test_the_query_is_the_restated_plan_on_both_sides_of_every_seam(lib):
    ncu = device_ncu()
    n = 0
    for C in (16, 32):
        CB = C // 16
        assert lib_plan(lib, PACK, 0, 0, 0, C) == [K_PACK, CB, 0, RR.pack_grid(C), 0, 0, 0, 0, 0, 0, 0]
        for H in HS:
            for W in WS:
                for B in BS:
                    assert RR.shape_ok(B, H, W, C)
                    assert lib_plan(lib, DGRAD, B, H, W, C) == [K_DGRAD, CB, 0, RR.dgrad_grid(B, H, W), 0, RR.nstrips(W), RR.cdiv(H, RR.DGRAD_ROWS), 0, 0, 0, 0], (B, H, W, C)
                    nblk = RR.wgrad_blocks(B, H, W, ncu)
                    assert lib_plan(lib, WGRAD, B, H, W, C) == [K_WGRAD, CB, 0, nblk, RR.wg_lds(CB), W // 64, H // 8, RR.wgrad_ntiles(B, H, W), RR.wfinish_grid(C),
                                                                  RR.chain_blocks(C), 3], (B, H, W, C)
                    assert lib.sgx_rgbconv_wgrad_ws_bytes(B, H, W, C) == RR.wgrad_ws_bytes(nblk, C) == (nblk + 1) * 48 * C * 4                    # (b)
                    for v in (0, 1, 2):
                        assert lib.sgx_rgbconv_tune(v, 0, 0) == 0
                        q = lib_plan(lib, FWD, B, H, W, C, 1)
                        if v == 0:
                            g = RR.fwdblur_geom(B, H, W)
                            assert q == [K_FWDBLUR, CB, 1, g.grid, 0, RR.nstrips(W), g.nrb, g.nit, 0, 0, 0], (B, H, W, C, q)
                        elif v == 1:
                            persistent_fwd(q, B, H, W, CB, 1, ncu)                                                                             # (c)
                        else:
                            f, nt = RR.rc_fwd(CB, 1), RR.fwd_ntiles(B, H, W, CB, 1)
                            assert q == [K_FWD, CB, 1, RR.ceil8(nt), f.LDS, W // f.TW, H // f.TH, nt, 0, 0, 0], (B, H, W, C, q)
                        persistent_fwd(lib_plan(lib, FWD, B, H, W, C, 0), B, H, W, CB, 0, ncu)                 # the plain convolution, under every variant
                        n += 1
    assert n == 2 * len(HS) * len(WS) * len(BS) * 3
    assert {W % RR.STRIP == 0 for W in WS} == {False, True} and [RR.nstrips(W) for W in WS] == [5, 10, 14, 32, 74]
    assert lib.sgx_rgbconv_tune(-1, 0, 0) == 0
    # LDS of rgbconv_fwd_kernel<CB, EPI> for <1, 0>, <1, 1>, <2, 0>, <2, 1>
    got = []
    for C, epi in ((16, 0), (16, 1), (32, 0), (32, 1)):
        assert lib.sgx_rgbconv_tune(1 if epi else 0, 0, 0) == 0
        got.append(lib_plan(lib, FWD, 1, 16, 64, C, epi)[4])
    assert got == [9552, 48928, 9552, 48800], got


def test_the_row_block_heuristic_steps_where_the_rule_says(lib):
    """fwdblur at 1024^2: B * 74 strips * ceil(1024 / (6 nit - 2)) row blocks against 3 * 256 * 24 waves."""
    want = {4: 3, 5: 3, 6: 4, 7: 5, 8: 5, 9: 6, 32: 6}
    for B, nit in want.items():
        g = RR.fwdblur_geom(B, 1024, 1024)
        assert g.nit == nit, (B, g)
        for C in (16, 32):
            assert lib_plan(lib, FWD, B, 1024, 1024, C, 1) == [K_FWDBLUR, C // 16, 1, g.grid, 0, 74, g.nrb, nit, 0, 0, 0], (B, C)
    for nit in (4, 5, 6):                                    # the step itself: the first B whose launch is large enough for nit
        B = min(b for b, v in want.items() if v >= nit)
        assert B * 74 * RR.cdiv(1024, 6 * nit - 2) >= 3 * 256 * 24 > (B - 1) * 74 * RR.cdiv(1024, 6 * nit - 2), (nit, B)
    # every override of sgx_rgbconv_tune
    for nit in range(1, 9):
        assert lib.sgx_rgbconv_tune(0, nit, 0) == 0
        for B, H, W, C in ((1, 48, 128, 16), (2, 48, 192, 32), (32, 1024, 1024, 16)):
            g = RR.fwdblur_geom(B, H, W, nit)
            assert g.nit == nit and lib_plan(lib, FWD, B, H, W, C, 1) == [K_FWDBLUR, C // 16, 1, g.grid, 0, RR.nstrips(W), g.nrb, nit, 0, 0, 0], (nit, B, H, W, C)
    assert lib.sgx_rgbconv_tune(-1, 0, 0) == 0
    assert lib_plan(lib, FWD, 1, 48, 128, 16, 1)[7] == 3


def test_wgrad_blocks_on_both_sides_of_three_per_cu(lib):
    ncu = device_ncu()
    per_image = (64 // 8) * (512 // 64)
    for B in (11, 12, 13, 3 * ncu // per_image, 3 * ncu // per_image + 1, 3 * ncu // per_image + 2):
        for C in (16, 32):
            q = lib_plan(lib, WGRAD, B, 64, 512, C)
            nt, nblk = B * per_image, RR.ceil8(min(B * per_image, 3 * ncu))
            assert (q[3], q[7], q[10]) == (nblk, nt, 3) and nblk == RR.wgrad_blocks(B, 64, 512, ncu), (B, C, q)
            assert lib.sgx_rgbconv_wgrad_ws_bytes(B, 64, 512, C) == (q[3] + 1) * 48 * C * 4
    if ncu == RR.NCU_NOMINAL:
        assert [tuple(lib_plan(lib, WGRAD, B, 64, 512, 16)[i] for i in (7, 3)) for B in (11, 12, 13)] == [(704, 704), (768, 768), (832, 768)]
    # the workspace query keeps its own, wider validity rule: it answers for H = 8, which the entry points refuse
    assert lib.sgx_rgbconv_wgrad_ws_bytes(1, 8, 64, 16) == (8 + 1) * 48 * 16 * 4 and lib.sgx_rgbconv_ok(1, 8, 64, 16, 1) == 0


def test_every_row_gets_its_kernels_and_geometry_from_the_query(lib):
    ncu = device_ncu()
    seen = set()
    for c0 in RR.CASES:
        c = RR.resolve(c0, ncu)
        a = c.args
        B, H, W, C = a.get("B") or 0, a.get("H") or 0, a.get("W") or 0, a["C"]
        epi = a.get("epi", 0)
        try:
            if c.entry == "sgx_rgbconv_fwd":
                assert lib.sgx_rgbconv_tune(a["variant"], a["nit"], 0) == 0
            if a.get("special") == "persistent":             # the batch size comes from the full grid, as in the GPU row
                per_image = RR.fwd_ntiles(1, H, W, C // 16, epi)
                probe = lib_plan(lib, FWD, RR.cdiv(4 * ncu, per_image), H, W, C, epi)
                B = RR.persistent_batch(probe[3], per_image)
                c = c._replace(args=dict(a, B=B))
            q = lib_plan(lib, ENTRY[c.entry], B, H, W, C, epi)
        finally:
            assert lib.sgx_rgbconv_tune(-1, 0, 0) == 0
        kernels, launches = launches_of(q)
        want_k, want_l = RR.plan(c, ncu)
        assert kernels == tuple(want_k) == c.kernels, (c.id, q)
        assert len(launches) == len(want_l), (c.id, q)
        for got, want in zip(launches, want_l):
            assert got[1:] == want[1:] and (want[0] is None or got[0] == want[0]), (c.id, q, want_l)
        if want_l[0][0] is None:                             # rgbconv_fwd_kernel's persistent grid: by value, from the reported occupancy
            persistent_fwd(q, B, H, W, C // 16, epi, ncu)
            if a.get("special") == "persistent":
                assert q[3] == probe[3] < q[7], (c.id, q, probe)
                if q[10] >= 2:                               # (without a device the occupancy reads 1, and 256 tiles per image give every block two)
                    assert {1, 2} <= set(RR.sched_counts(q[3], q[7])), (c.id, q)
        seen.add((q[0], q[1], q[2]))
    assert seen == {(K_PACK, 1, 0), (K_PACK, 2, 0), (K_FWD, 1, 0), (K_FWD, 2, 0), (K_FWD, 1, 1), (K_FWD, 2, 1), (K_FWDBLUR, 1, 1), (K_FWDBLUR, 2, 1), (K_DGRAD, 1, 0),
                    (K_DGRAD, 2, 0), (K_WGRAD, 1, 0), (K_WGRAD, 2, 0)}, seen


def rejected(L, entry, B, H, W, C, epi, code, words):
    out = (ctypes.c_int * PLAN_INTS)(*([7] * PLAN_INTS))
    L.sgx_clear_error()
    rc = L.sgx_rgbconv_plan(entry, B, H, W, C, epi, ctypes.addressof(out))
    msg = L.sgx_last_error().decode(errors="replace")
    L.sgx_clear_error()
    assert rc == code and words in msg and list(out) == [0] * PLAN_INTS, (entry, B, H, W, C, epi, rc, msg, list(out))


def test_rejections(lib):
    for B, H, W, C in REFUSED:
        assert lib.sgx_rgbconv_ok(B, H, W, C, 1) == 0 and not RR.shape_ok(B, H, W, C)
        for entry in (FWD, DGRAD, WGRAD):
            rejected(lib, entry, B, H, W, C, 1, RR.EUNSUPPORTED, "sgx_rgbconv_ok == 0")
    rejected(lib, PACK, 0, 0, 0, 24, 0, RR.EUNSUPPORTED, "16 or 32 channels")
    for entry in (-1, 4):
        rejected(lib, entry, 1, 16, 64, 16, 1, RR.EINVAL, f"rgbconv_plan: entry {entry}")
    rejected(lib, FWD, 1, 16, 64, 16, 2, RR.EINVAL, "epilogue 2")
    lib.sgx_clear_error()
    assert lib.sgx_rgbconv_plan(FWD, 1, 16, 64, 16, 1, None) == RR.EINVAL and b"out is NULL" in lib.sgx_last_error()
    lib.sgx_clear_error()
