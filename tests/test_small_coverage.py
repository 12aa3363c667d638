"""CPU side of tests/test_gpu_small_paths.py: (a) every hipLaunchKernelGGL site of csrc/small.hip outside the streaming part is claimed by a row of
small_ref.CASES, every instantiation the launchers can reach is named by a row, and the kernel branches the rows are there for are reached by
their shapes; (b) sgx_gemm_ws_bytes, which launches nothing, agrees with the restated gemm_splits on both sides of its seams; (c) a row's kernel
list is what the restated rules give for its arguments; the contract rejections return before any launch; (d) the criteria pass an fp32
emulation of the kernels' own summation order and fail six planted errors -- with the rel-L2 each causes, and whether the suite's older
whole-tensor tolerance would have let it through."""
import collections
import os
import re

import numpy as np
import pytest
import torch

import epilogue_ref as ER
import gpu_util
import small_ref as SM
import streaming_ref as SR
import test_streaming_coverage as TSC
from oracle import stylegan_oracle as O

SMALL = os.path.join(TSC.CSRC, "small.hip")
F32 = torch.float32


@pytest.fixture(scope="module")
def lib():
    from stylegan.pytorch_amd import native
    native.build()
    return native.lib()


def source():
    with open(SMALL) as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------------------- (a) the scan
def sites():
    return [s for s in TSC.launch_sites(SMALL) if s[0] not in SR.SMALL_HIP_COVERED]


def test_every_launch_site_of_small_hip_has_a_row():
    sm = sites()
    assert len(sm) == 10, len(sm)                           # 15 in the file, 5 of them the streaming part's: one site per kernel of KERNELS,
    assert sorted(s[0] for s in sm) == sorted(SM.KERNELS)   # ... mbstd 3, the GEMM's 3, the style affines 3, the logistic head 1
    assert TSC.unclaimed(sm, SM.CASES, {}) == []
    # the tile kernel's one site is generic in U of sgx_by_int<1, 8>: the list is read from the source, and both values are named by rows
    (tile,) = [s for s in sm if s[0] == "gemm_f32_kernel"]
    held = [f"gemm_f32_kernel<{v}>" for v in tile[2]["U"]]
    named = {k for c in SM.CASES for k in c.kernels}
    assert tile[1] == "<U>" and held == [SM.K1, SM.K8] and set(held) <= named
    # every __global__ function of the file belongs to this table or to the streaming one, and every kernel a row names exists
    kernels = set(re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+([A-Za-z_0-9]+)", source()))
    assert kernels == set(SM.KERNELS) | set(SR.SMALL_HIP_COVERED), kernels ^ (set(SM.KERNELS) | set(SR.SMALL_HIP_COVERED))
    assert {k.split("<")[0] for k in named} == set(SM.KERNELS)
    for c in SM.CASES:
        assert c.why and c.entry in SM.ROWS, c.id
    assert dict(collections.Counter(c.entry for c in SM.CASES)) == SM.ROWS
    assert len({r[0] for r in SM.REJECTIONS}) == len(SM.REJECTIONS)


def test_a_new_site_or_a_dropped_row_is_noticed():
    sm = sites()
    assert TSC.unclaimed(sm + [("style_fwd_kernel", "<64>")], SM.CASES, {}) == ["style_fwd_kernel<64>"]
    assert TSC.unclaimed(sm + [("gemm_batched_kernel", "")], SM.CASES, {}) == ["gemm_batched_kernel"]
    no_bf16_bwd2 = [c for c in SM.CASES if c.kernels != ("mbstd_bwd2_kernel<bf16_t>",)]
    assert TSC.unclaimed(sm, no_bf16_bwd2, {}) == ["mbstd_bwd2_kernel<T> for ['bf16_t']"]
    no_b32 = [c for c in SM.CASES if not (c.entry == "sgx_style_bwd_data" and c.args["B"] > 16)]
    assert TSC.unclaimed(sm, no_b32, {}) == ["style_bwd_data_kernel<MB> for [32]"]
    # ... and either instantiation of the tile GEMM, now one site
    assert TSC.unclaimed(sm, [c for c in SM.CASES if SM.K8 not in c.kernels], {}) == ["gemm_f32_kernel<U> for [8]"]
    assert TSC.unclaimed(sm, [c for c in SM.CASES if SM.K1 not in c.kernels], {}) == ["gemm_f32_kernel<U> for [1]"]


def test_rows_reach_the_branches_they_are_there_for():
    """The kernel bodies and loop shapes behind one launch site, from the rules on the rows' own arguments."""
    gem = [c for c in SM.CASES if c.entry in ("sgx_gemm_f32", "sgx_linear_fwd", "sgx_linear_bwd_data", "sgx_linear_bwd_param")]
    pls = [(c, SM.gemm_plan_of(c)) for c in gem]
    ints = [(c, pl) for c, pl in pls if c.args["data"] == "int"]
    tile = [(c, pl) for c, pl in ints if pl.body is not None]
    assert {pl.body for _, pl in tile} == {(va, vb, mk) for va in (False, True) for vb in (False, True) for mk in (False, True)} - {(False, True, True), (True, True, True)}
    # (MASK with VB does not exist: the only masked GEMMs are t00 and t10)
    assert any(pl.tail for _, pl in tile) and any(not pl.tail for _, pl in tile)
    assert {pl.kernels for _, pl in ints} == {(SM.OUTER,), (SM.K1,), (SM.K8,), (SM.K1, SM.REDUCE), (SM.K8, SM.REDUCE)}
    # vector bodies are only entered by a full 16-k step: each of VA and VB has an integer row with one
    full = lambda c, pl: any(ke - kb >= 16 for z in SM.gemm_slices(pl_K(c), pl.splits) for kb, ke in z)
    assert any(pl.body[0] and full(c, pl) for c, pl in tile) and any(pl.body[1] and full(c, pl) for c, pl in tile)
    assert any(pl.body == (True, False, True) and full(c, pl) for c, pl in tile) and any(pl.body == (False, False, True) for c, pl in tile)
    # <8> rows with an 8-step trip (a slice of 128 or more), with and without a remainder behind it
    k8 = [(c, pl) for c, pl in ints if SM.K8 in pl.kernels]
    assert any(pl.kper == 128 for _, pl in k8) and any(pl.kper > 128 and pl.kper % 128 for _, pl in k8)
    # split-K: an uneven last split, an empty last split, an empty wave slice inside a non-empty split; 8200 is what the issue computed
    by = SM.BY_ID
    sl = SM.gemm_slices(8200, SM.gemm_splits(5, 15, 8200))
    assert len(sl) == 32 and sl[31][0][0] == 31 * 272 > 8200 and all(kb >= ke for kb, ke in sl[31])
    assert sl[30][0] == (8160, 8176) and sl[30][2] == (8192, 8200) and sl[30][3][0] > sl[30][3][1]
    assert by["gemm-5x15x8200-t00-int"].kernels == (SM.K1, SM.REDUCE)
    sl = SM.gemm_slices(1025, 4)
    assert sl[3][0][0] == 816 and max(ke for _, ke in sl[3]) == 1025
    assert SM.gemm_plan_of(by["gemm-16x20x1025-t00-int-wsnull"]).splits == 1 and SM.gemm_plan_of(by["gemm-5x16x1030-t10-int-wsshort"]).splits == 1
    # colsum: the 8-at-a-time loop with and without a remainder, the remainder alone
    par = [c.args["B"] for c in gem if c.entry == "sgx_linear_bwd_param" and c.args["db"]]
    assert any(b < 8 for b in par) and any(b >= 8 and b % 8 for b in par)
    assert any(b % 8 == 0 for b in par) and any(not c.args["db"] and c.args["mask"] for c in gem if c.entry == "sgx_linear_bwd_param")
    # style: every MB per entry point, style_group's two arms, ragged tiles, D below 512, NULL bias / db, untouched layers, the pipeline's shapes
    for e in ("sgx_style_fwd", "sgx_style_bwd_data", "sgx_style_bwd_param"):
        rows = [c for c in SM.CASES if c.entry == e]
        assert {SM.style_mb(c.args["B"]) for c in rows} == {4, 8, 16, 32}
        assert {SM.style_mb(c.args["B"]) for c in rows if c.args["data"] == "int"} == {4, 8, 16, 32}
        assert any(len(c.args["Ns"]) > 64 for c in rows) and any(1 < len(c.args["Ns"]) <= 64 for c in rows)
        assert any(n % 16 for c in rows for n in c.args["Ns"]) and {64, 128, 512} == {c.args["D"] for c in rows}
        assert any(not c.args["bias"] for c in rows) and any(not c.args["db"] for c in rows) and any(len(c.args["Ns"]) < c.args["L"] for c in rows)
        assert all(len(set(c.args["layers"])) == len(c.args["Ns"]) and max(c.args["layers"]) < c.args["L"] for c in rows)
    full4 = {SM.style_full_chunks(n) for c in SM.CASES if c.entry == "sgx_style_bwd_data" and c.args["B"] <= 8 for n in c.args["Ns"]}
    assert {0, 1, 3, 4} <= full4, full4
    assert SM.style_full_chunks(2, 2) == 0 and SM.style_full_chunks(2, 3) == 0
    assert max(SM.style_plan("sgx_style_bwd_data", c.args["B"], c.args["D"], c.args["Ns"])[1][0][2] for c in SM.CASES if c.entry == "sgx_style_bwd_data") == 32 * 1024 * 4
    # mbstd: B = 1, 2, 3, 4, 8, 12; the unrolled loops end before, at, inside and after a trip; both dtypes for the three kernels
    mb = [c for c in SM.CASES if c.entry.startswith("sgx_mbstd")]
    assert {c.args["B"] for c in mb} == {1, 2, 3, 4, 8, 12} and {c.args["Cpad"] - c.args["C"] for c in mb} == {1, 8}
    n = {c.args["HW"] * c.args["C"] for c in mb}
    assert any(v < SM.MBSTD_BATCH for v in n) and SM.MBSTD_BATCH in n and any(v > SM.MBSTD_BATCH and v % SM.MBSTD_BATCH for v in n)
    assert {(c.entry, c.dtype) for c in mb} == {(e, t) for e in ("sgx_mbstd_fwd", "sgx_mbstd_bwd", "sgx_mbstd_bwd2") for t in (SM.F, SM.H)}
    lg = [c for c in SM.CASES if c.entry == "sgx_logistic_loss"]
    assert {c.args["nf"] for c in lg if not c.args.get("special")} == {1, 63, 64, 65, 200} and all(c.args["nf"] != c.args["nr"] for c in lg)
    s20 = np.float32(20)
    assert SM.SPECIAL_LOGITS[1] > 20 > SM.SPECIAL_LOGITS[2] and np.float32(SM.SPECIAL_LOGITS[1]) == np.nextafter(s20, np.float32(30))


def pl_K(c):
    a = c.args
    return {"sgx_gemm_f32": a.get("K"), "sgx_linear_fwd": a.get("K"), "sgx_linear_bwd_data": a.get("N"), "sgx_linear_bwd_param": a.get("B")}[c.entry]


# ---------------------------------------------------------------------------------------------------------------- (b) the workspace query
def test_gemm_ws_bytes_is_the_restated_rule(lib):
    """Both sides of tiles = 256 (M x N tiles of 16), of K = 1024 and of the cap ceil(512 / tiles) on K / 256."""
    seen = set()
    for M in (1, 4, 16, 17, 33, 64, 255 * 16, 256 * 16):
        for Nn in (4, 15, 16, 17, 512, 4080, 4096, 4097, 8192):
            for K in (1, 512, 1023, 1024, 1025, 1279, 1280, 4096, 4112, 8192, 8200, 1 << 17, 131073):
                want = SM.gemm_ws_bytes(M, Nn, K)
                assert lib.sgx_gemm_ws_bytes(M, Nn, K) == want, (M, Nn, K)
                tiles = SM.cdiv(M, 16) * SM.cdiv(Nn, 16)
                seen.add((tiles >= 256, K >= 1024, K // 256 > SM.cdiv(512, tiles), want > 0))
    assert (True, True, True, False) in seen and (False, False, False, False) in seen and (False, True, True, True) in seen and (False, True, False, True) in seen
    assert SM.gemm_splits(1, 4096, 1024) == 1 and SM.gemm_splits(1, 4080, 1024) == 3 and SM.gemm_splits(4, 512, 8192) == 16 and SM.gemm_splits(5, 15, 8200) == 32


# ---------------------------------------------------------------------------------------------------------------- (c) table against rules
def test_each_rows_kernel_list_is_what_the_rules_give():
    for c in SM.CASES:
        kernels, launches = SM.plan(c)
        assert tuple(kernels) == c.kernels, (c.id, kernels, c.kernels)
        assert len(launches) == len(kernels) and all(g[0] >= 1 and g[1] >= 1 and g[2] >= 1 for g, _, _ in launches), c.id
    mbs = {c.id: SM.plan(c)[1][0][0] for c in SM.CASES if c.entry == "sgx_mbstd_fwd"}
    assert mbs["mbstd_fwd-f32-B12-HW9-C1000-pad8-rnd"] == (3, 8, 1) and mbs["mbstd_fwd-f32-B3-HW16-C40-pad1-rnd"] == (1, 8, 1)


def test_references_alone_integer_rows_are_exact_and_kink_counts_stay_under_the_cap():
    """What the GPU rows rely on, checked on the CPU operands: an integer row's exact value is an fp32 number and no partial sum can leave
    the exact range; a LeakyReLU row's reference has at most kink_cap pre-activations inside the window."""
    for c in SM.CASES:
        if c.entry == "sgx_linear_fwd":
            o, pl = SM.gemm_operands(c), SM.gemm_plan_of(c)
            pre, S = SM.linear_fwd(o["x"].double(), o["w"].double(), None if o["bias"] is None else o["bias"].double(), o["w_mul"], o["b_mul"])
            if c.args["act"] and c.args["data"] != "int":            # (an integer row is compared bit for bit: no window)
                n =SM.gemm_chain(pl, bias=c.args["bias"], act=True)
                assert SM.kink_count(pre, S, n) <= ER.kink_cap(pre.numel()), c.id
            if c.args["data"] == "int":
                assert torch.equal(pre.float().double(), pre) and float(S.max()) / o["w_mul"] < 2 ** 24, c.id
        if c.entry == "sgx_gemm_f32" and c.args["data"] == "int" and c.args["M"] * c.args["N"] <= 1 << 16:
            o = SM.gemm_operands(c)
            ref, S = SM.gemm(o["A"].double(), o["B"].double(), c.args["ta"], c.args["tb"], o["alpha"])
            assert torch.equal(ref.float().double(), ref) and float(S.max()) / o["alpha"] < 2 ** 24, c.id
    assert 9 * 8200 < 2 ** 24


def test_mbstd_references_are_the_derivatives_of_the_oracle():
    """small_ref's closed forms against autograd through oracle.minibatch_stddev, first and second order."""
    for B in (1, 3, 8):
        HW, C = 6, 5
        x = SM.rnd((B, HW, C), 1).double().requires_grad_(True)
        w = SM.rnd((B, HW, C + 1), 2).double()
        gg = SM.rnd((B, HW, C), 3).double()
        nchw = lambda t: t.permute(0, 2, 1).unsqueeze(-1)
        y = O.minibatch_stddev(nchw(x)).squeeze(-1).permute(0, 2, 1)                            # [B][HW][C + 1]
        st = SM.mbstd_stats(x.detach())
        assert torch.allclose(y[..., C], st.stat.repeat(st.G).view(B, 1).expand(B, HW), rtol=1e-12, atol=0)
        wv = w.clone().requires_grad_(True)
        (dx,) = torch.autograd.grad((y * wv).sum(), x, create_graph=True)
        ref, bound = SM.mbstd_bwd(w, x.detach(), C)
        assert torch.allclose(dx, ref, rtol=1e-10, atol=1e-12) and bool((bound > 0).all())
        gx, gw = torch.autograd.grad((dx * gg).sum(), (x, wv))
        dstat, dstat_b, rg, bg = SM.mbstd_bwd2(gg, w, x.detach(), C)
        assert torch.allclose(gx, rg, rtol=1e-9, atol=1e-11), B
        assert torch.allclose(gw[..., :C], gg) and torch.allclose(gw[..., C], dstat.repeat(st.G).view(B, 1).expand(B, HW), rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- rejections
FAKE, ODD = 0x10000, 0x10004                                 # device pointers that are never followed: 16-byte aligned, and 4 bytes off


def reject(L, id):
    P, st = FAKE, None
    calls = {
        "gemm-M0": lambda: L.sgx_gemm_f32(P, P, P, 0, 16, 16, 0, 0, 1.0, None, 0, st),
        "gemm-K-negative": lambda: L.sgx_gemm_f32(P, P, P, 4, 16, -1, 0, 0, 1.0, None, 0, st),
        "linear_fwd-N0": lambda: L.sgx_linear_fwd(P, P, P, P, 4, 0, 16, 1.0, 1.0, 0, st),
        "linear_bwd_data-B0": lambda: L.sgx_linear_bwd_data(P, P, P, P, 0, 16, 16, 1.0, st),
        "linear_bwd_param-K0": lambda: L.sgx_linear_bwd_param(P, P, P, P, P, 4, 16, 0, 1.0, 1.0, st),
        "mbstd_fwd-B6": lambda: L.sgx_mbstd_fwd(P, P, 6, 16, 8, 9, 0, st),
        "mbstd_bwd-B6": lambda: L.sgx_mbstd_bwd(P, P, P, 6, 16, 8, 9, 0, st),
        "mbstd_bwd2-B6": lambda: L.sgx_mbstd_bwd2(P, P, P, P, P, 6, 16, 8, 9, 1, st),
        "mbstd_fwd-Cpad-eq-C": lambda: L.sgx_mbstd_fwd(P, P, 4, 16, 8, 8, 0, st),
        "mbstd_bwd-Cpad-lt-C": lambda: L.sgx_mbstd_bwd(P, P, P, 4, 16, 8, 7, 1, st),
        "mbstd_bwd2-Cpad-eq-C": lambda: L.sgx_mbstd_bwd2(P, P, P, P, P, 4, 16, 8, 8, 0, st),
        "mbstd_fwd-dtype2": lambda: L.sgx_mbstd_fwd(P, P, 4, 16, 8, 9, 2, st),
        "mbstd_bwd-dtype2": lambda: L.sgx_mbstd_bwd(P, P, P, 4, 16, 8, 9, 2, st),
        "mbstd_bwd2-dtype2": lambda: L.sgx_mbstd_bwd2(P, P, P, P, P, 4, 16, 8, 9, 2, st),
        "style_fwd-B33": lambda: L.sgx_style_fwd(P, P, P, 2, 33, 512, 4, st),
        "style_bwd_data-B33": lambda: L.sgx_style_bwd_data(P, P, P, 2, 33, 512, 32, st),
        "style_bwd_param-B33": lambda: L.sgx_style_bwd_param(P, P, P, P, P, 2, 33, 512, 4, st),
        "style_fwd-D96": lambda: L.sgx_style_fwd(P, P, P, 2, 4, 96, 4, st),
        "style_bwd_data-D96": lambda: L.sgx_style_bwd_data(P, P, P, 2, 4, 96, 32, st),
        "style_bwd_param-D96": lambda: L.sgx_style_bwd_param(P, P, P, P, P, 2, 4, 96, 4, st),
        "style_fwd-lm-misaligned": lambda: L.sgx_style_fwd(ODD, P, P, 2, 4, 512, 4, st),
        "logistic-fake-null": lambda: L.sgx_logistic_loss(None, 4, P, 4, 1.0, 0, P, P, P, st),
        "logistic-nf0": lambda: L.sgx_logistic_loss(P, 0, P, 4, 1.0, 0, P, P, P, st),
        "logistic-g-with-real": lambda: L.sgx_logistic_loss(P, 4, None, 1, 1.0, 1, P, P, None, st),
        "logistic-d-real-null": lambda: L.sgx_logistic_loss(P, 4, None, 4, 1.0, 0, P, P, P, st),
        "logistic-d-g_real-null": lambda: L.sgx_logistic_loss(P, 4, P, 4, 1.0, 0, P, P, None, st),
        "logistic-d-nr0": lambda: L.sgx_logistic_loss(P, 4, P, 0, 1.0, 0, P, P, P, st),
    }
    return calls[id]()


@pytest.mark.parametrize("id,entry,code,words,why", SM.REJECTIONS, ids=[r[0] for r in SM.REJECTIONS])
def test_contract_rejections_return_before_any_launch(lib, id, entry, code, words, why):
    lib.sgx_clear_error()
    rc = reject(lib, id)
    msg = lib.sgx_last_error().decode(errors="replace")
    lib.sgx_clear_error()
    assert rc == code and words in msg, (id, rc, msg, why)


# ---------------------------------------------------------------------------------------------------------------- (d) the criteria on emulations
f4 = np.float32


def emu_gemm(A, Bm, alpha, drop_last_k=False, skip_wave=None):
    """gemm_f32_kernel, one split, in numpy fp32: each wave adds the products of its K slice in k order (one admissible order of the MFMA's
    sums), the partials meet as ((w0 + w1) + w2) + w3, then alpha.  A [M][K], B [K][N]."""
    (M, K), Nn = A.shape, Bm.shape[1]
    parts = []
    sl = SM.gemm_slices(K, 1)[0]
    tails = [w for w, (kb, ke) in enumerate(sl) if ke > kb and (ke - kb) % 16]
    for w, (kb, ke) in enumerate(sl):
        acc = np.zeros((M, Nn), f4)
        hi = ke - 1 if drop_last_k and tails and w == tails[-1] else ke
        for k in range(kb, hi):
            acc = acc + A[:, k:k + 1] * Bm[k:k + 1, :]
        parts.append(np.zeros_like(acc) if w == skip_wave else acc)
    return f4(alpha) * (((parts[0] + parts[1]) + parts[2]) + parts[3])


def emu_colsum(A, cscale, no_remainder=False):
    """colsum of gemm_f32_kernel: a sequential fp32 sum over k.  A [rows][K]."""
    K = A.shape[1]
    t = np.zeros(A.shape[0], f4)
    for k in range(K // 8 * 8 if no_remainder else K):
        t = t + A[:, k]
    return f4(cscale) * t


def emu_style_fwd(x, W, bias, w_mul, b_mul, clamp_at=None):
    """style_fwd_kernel in numpy fp32: lane kl of 16 adds its D / 64 pieces ((p + p) + (p + p)) in k order, four xor-shuffle adds, w_mul * acc +
    b_mul * bias.  clamp_at: the planted row clamp (n < clamp_at ? n : clamp_at - 1) in place of the kernel's N."""
    N_, D = W.shape
    rows = np.arange(N_)
    if clamp_at is not None:
        rows = np.where(rows < clamp_at, rows, clamp_at - 1)
    Wp = W[rows].reshape(N_, D // 64, 16, 4)
    xp = x.reshape(x.shape[0], 1, D // 64, 16, 4)
    pr = Wp[None] * xp                                                                      # [B][N][u][kl][4]
    piece = (pr[..., 0] + pr[..., 1]) + (pr[..., 2] + pr[..., 3])
    acc = np.zeros(piece.shape[:2] + (16,), f4)
    for u in range(D // 64):
        acc = acc + piece[:, :, u]
    for o in (8, 4, 2, 1):
        acc = acc + acc[..., np.arange(16) ^ o]
    return f4(w_mul) * acc[..., 0] + f4(b_mul) * bias


def emu_mbstd_fwd(x, Cpad, pad_holds_stat=False, member_from_0=None):
    """mbstd_fwd_kernel on fp32 torch tensors: mbstd_std's chain per element, the mean of s in fp64 rounded once, the padded copy."""
    B, HW, C = x.shape
    G = min(B, 4)
    M = B // G
    v = x.reshape(G, M, HW, C).clone()
    if member_from_0 is not None:
        v[member_from_0] = v[0]
    mu = v[0].clone()
    for g in range(1, G):
        mu = mu + v[g]
    mu = mu / G
    var = torch.zeros_like(mu)
    for g in range(G):
        dlt = v[g] - mu
        var = var + dlt * dlt
    s = torch.sqrt(var / G + torch.tensor(1e-8, dtype=F32))
    stat = (s.double().sum((1, 2)) / (HW * C)).float()                                      # [M]
    y = torch.zeros(B, HW, Cpad, dtype=x.dtype)
    y[..., :C] = x
    col = stat.repeat(G).view(B, 1)
    y[..., C] = col
    if pad_holds_stat:
        y[..., C + 1] = col
    return y


def _report(name, rel, tol, old):
    passes = rel <= tol
    print(f"planted {name}: rel-L2 {rel:.3e} against the older tolerance {tol:.0e} ({old}): {'passes' if passes else 'fails'} there")
    return passes


def test_criteria_pass_the_emulations_and_fail_the_six_planted_errors():
    """The honest fp32 emulation meets each criterion; each planted error fails it with an index in the message.  What the rel-L2 tests that
    held this code before make of the same tensors is printed and pinned.  Five of the six are gross enough for a whole-tensor norm had those
    tests run the shape -- they did not: no ragged style group, no G = 3, no colsum remainder (at their B = 8 the planted loop is the whole
    loop, asserted below) -- and the padding column passes there at any shape, because those tests look at the first C + 1 channels only."""
    old = {}
    # ---- GEMM, 37 x 50 x 77 t00 (a shape of test_gemm_paths_match_fp64, tolerance 2e-5): slices of 32, 32, 13
    M, Nn, K, alpha = 37, 50, 77, SR.f32(0.37)
    A, Bm = SM.rnd((M, K), 11).numpy(), SM.rnd((K, Nn), 12).numpy()
    ref, S = SM.gemm(torch.from_numpy(A).double(), torch.from_numpy(Bm).double(), 0, 0, alpha)
    n = SM.gemm_chain(SM.gemm_plan(M, Nn, K, 0, 0))
    assert n == 32 + 3 + 1
    assert SR.assert_elementwise(torch.from_numpy(emu_gemm(A, Bm, alpha)), ref, S, n, F32, "gemm") <= 1.0
    bad = torch.from_numpy(emu_gemm(A, Bm, alpha, drop_last_k=True))
    with pytest.raises(AssertionError, match=r"of 1850 elements outside the bound; first at flat index 0 \(0, 0\)"):
        SR.assert_elementwise(bad, ref, S, n, F32, "last k of the K tail dropped")
    old["tail-k"] = _report("last k of the K tail dropped", gpu_util.rel_err(bad, ref), 2e-5, "test_gemm_paths_match_fp64")
    bad = torch.from_numpy(emu_gemm(A, Bm, alpha, skip_wave=2))
    with pytest.raises(AssertionError, match=r"outside the bound; first at flat index 0 "):
        SR.assert_elementwise(bad, ref, S, n, F32, "wave 2's partial omitted")
    old["wave"] = _report("one wave's partial omitted from the LDS reduce", gpu_util.rel_err(bad, ref), 2e-5, "test_gemm_paths_match_fp64")
    # ---- colsum at B = 9 (sgx_linear_bwd_param: K of the GEMM = batch): db[N] = b_mul sum_b gy[b][n]; the older test runs B = 4 and 8
    Bt, Nl = 9, 36
    gy = SM.rnd((Bt, Nl), 24).numpy()
    rb, Sb = SR.f32(1.3) * torch.from_numpy(gy).double().sum(0), SR.f32(1.3) * torch.from_numpy(gy).double().abs().sum(0)
    assert SR.assert_elementwise(torch.from_numpy(emu_colsum(gy.T.copy(), SR.f32(1.3))), rb, Sb, Bt + 2, F32, "colsum") <= 1.0
    bad = torch.from_numpy(emu_colsum(gy.T.copy(), SR.f32(1.3), no_remainder=True))
    with pytest.raises(AssertionError, match=r"36 of 36 elements outside the bound; first at flat index 0 "):
        SR.assert_elementwise(bad, rb, Sb, Bt + 2, F32, "colsum remainder loop missing")
    old["colsum"] = _report("colsum remainder loop missing (B = 9)", gpu_util.rel_err(bad, rb), 1e-5, "test_fused_linear_matches_torch")
    gy8 = gy[:8]
    assert np.array_equal(emu_colsum(gy8.T.copy(), 1.3), emu_colsum(gy8.T.copy(), 1.3, no_remainder=True))       # ... at B = 8 there is nothing to miss
    # ---- style_fwd with a ragged last tile: N = 1030 of the older test's magnitude (its groups are multiples of 16), B = 4, D = 512
    Bs, D, Ns = 4, 512, 1030
    x, W, bias = SM.rnd((Bs, D), 31).numpy(), SM.rnd((Ns, D), 40).numpy(), SM.rnd((Ns,), 140).numpy()
    wm, bm = SR.f32(0.37), SR.f32(1.3)
    ry, Sy = SM.style_fwd(torch.from_numpy(x).double(), torch.from_numpy(W).double(), torch.from_numpy(bias).double(), wm, bm)
    ns = SM.style_chain("sgx_style_fwd", Bs, D, Ns)
    assert ns == 8 + 10
    assert SR.assert_elementwise(torch.from_numpy(emu_style_fwd(x, W, bias, wm, bm)), ry, Sy, ns, F32, "style_fwd") <= 1.0
    bad = torch.from_numpy(emu_style_fwd(x, W, bias, wm, bm, clamp_at=Ns - 1))
    with pytest.raises(AssertionError, match=r"4 of 4120 elements outside the bound; first at flat index 1029 \(0, 1029\)"):
        SR.assert_elementwise(bad, ry, Sy, ns, F32, "last row of the ragged tile from the clamped row")
    old["style-row"] = _report("last row of a ragged style tile taken from the clamped row", gpu_util.rel_err(bad, ry), 1e-5, "test_grouped_style_affines_match_per_layer_linears")
    # ---- mbstd forward, B = 3 (G = 3), HW = 16, C = 40, Cpad = 48
    xb = SM.rnd((3, 16, 40), 51) + 0.5
    st = SM.mbstd_stats(xb.double())
    y = emu_mbstd_fwd(xb, 48)
    assert SM.check_padded(y, xb, 40, st.stat, st.dstat, 3, 40, "mbstd") <= 1.0
    yref = y.double().clone()
    yref[..., 40] = st.stat.repeat(3).view(3, 1)
    bad = emu_mbstd_fwd(xb, 48, pad_holds_stat=True)
    with pytest.raises(AssertionError, match=r"48 padding elements are not \+0, first at \(0, 0, 0\)"):
        SM.check_padded(bad, xb, 40, st.stat, st.dstat, 3, 40, "padding column holds the statistic")
    old["pad"] = _report("an mbstd padding column holding the statistic", gpu_util.rel_err(bad[..., :41], yref[..., :41]), 1e-6, "the mbstd tests: StddevLayer returns the first C + 1 channels only")
    bad = emu_mbstd_fwd(xb, 48, member_from_0=2)
    with pytest.raises(AssertionError, match=r"1 of 1 values outside the bound; first at \(0,\)"):
        SM.check_padded(bad, xb, 40, st.stat, st.dstat, 3, 40, "member 2 read from image 0")
    old["member"] = _report("a group member read from image 0 for G = 3", gpu_util.rel_err(bad, yref), 1e-6, "the mbstd tests (none of which has G = 3)")
    # ---- an unwritten element (the Guarded prefill: every byte SENTINEL, a NaN) fails each of the three kinds of check
    nan = torch.full((4,), float("nan"))
    nan.view(torch.uint8)[:] = SR.SENTINEL
    one = torch.ones(4, dtype=torch.float64)
    for chk in (lambda: SM.assert_bits(nan, one, "sentinel"), lambda: SM.check_act(nan, one, one, 1000, 1, "sentinel"), lambda: ER.assert_within(nan, one, 1e30 * one, "sentinel")):
        with pytest.raises(AssertionError, match="sentinel: 4 of 4 "):
            chk()
    assert old == {"tail-k": False, "wave": False, "colsum": False, "style-row": False, "pad": True, "member": False}, old
