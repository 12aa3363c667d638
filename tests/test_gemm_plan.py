"""CPU: what a call of the fp32 GEMM (sgx_gemm_f32, the three sgx_linear_*) will launch, asked of the library itself.  sgx_gemm_plan answers
from gemm_plan, the function gemm_launch of csrc/small.hip executes, so on a grid of shapes with points on both sides of every seam -- K = 4 / 5
and N % 4 (the outer product), 256 tiles, K = 1024, the cap ceil(512 / tiles) on K / 256, a split's K of 511 / 512 -- under both transposes,
every fusion, every alignment and a full, a short and no workspace: (a) kernel, splits, grids and vec are what tests/small_ref.py restates;
(b) sgx_gemm_ws_bytes is the split count of a full workspace; (c) every GEMM-family row of small_ref.CASES gets its kernel list from the query;
(d) a shape that is not positive is SGX_EINVAL.  The query is host-only: nothing here opens the GPU, and csrc/small.hip reads no environment
switch, so one process does."""
import ctypes

import pytest

import small_ref as SM

PLAN_INTS = 7
MS = (1, 4, 5, 16, 17, 64, 4080, 4096)
NS = (3, 4, 15, 16, 17, 512, 4080, 4096, 8192)
KS = (1, 4, 5, 8, 511, 512, 1023, 1024, 1025, 2047, 2048, 8192, 8200, 131072)
KINDS = {0: SM.OUTER, 1: SM.K1, 2: SM.K8}


@pytest.fixture(scope="module")
def lib():
    from stylegan.pytorch_amd import native
    native.build()
    return native.lib()


def lib_plan(L, M, N, K, ta, tb, fuse, ws_bytes, align):
    out = (ctypes.c_int * PLAN_INTS)()
    rc = L.sgx_gemm_plan(M, N, K, ta, tb, fuse, ws_bytes, align, ctypes.addressof(out))
    assert rc == 0, (M, N, K, ta, tb, fuse, ws_bytes, align, rc)
    return list(out)


def test_the_query_is_the_restated_plan_on_both_sides_of_every_seam(lib):
    seen, n = set(), 0
    for M in MS:
        for N in NS:
            for K in KS:
                need = SM.gemm_ws_bytes(M, N, K)
                full = lib_plan(lib, M, N, K, 0, 1, 0, need, 7)
                assert lib.sgx_gemm_ws_bytes(M, N, K) == (full[1] * M * N * 4 if full[1] > 1 else 0) == need, (M, N, K)         # (b)
                for ta in (0, 1):
                    for tb in (0, 1):
                        for fuse in range(4):
                            for ws in sorted({0, max(need - 4, 0), need}):
                                # the restatement takes "B and C aligned" (bits 1 and 2 of align) as one flag; vec is bits 0 and 1 as given
                                pls = {bc: SM.gemm_plan(M, N, K, ta, tb, mask=bool(fuse & 1), epi=bool(fuse & 2), ws_bytes=ws, aligned=bc) for bc in (False, True)}
                                for align in range(8):
                                    want = SM.gemm_plan_ints(pls[align & 6 == 6], align)
                                    assert lib_plan(lib, M, N, K, ta, tb, fuse, ws, align) == want, (M, N, K, ta, tb, fuse, ws, align)
                                    n += 1
                                seen.update((pl.kernels, pl.splits > 1, ws >= need > 0, bool(fuse & 2)) for pl in pls.values())
    assert n == 2 * 2 * 4 * 8 * sum(3 if SM.gemm_ws_bytes(M, N, K) else 1 for M in MS for N in NS for K in KS), n
    # every kernel list was met, and each reason for one split where the rule wants more: no workspace, a short one, a fused epilogue
    assert {k for k, _, _, _ in seen} == {(SM.OUTER,), (SM.K1,), (SM.K8,), (SM.K1, SM.REDUCE), (SM.K8, SM.REDUCE)}
    assert (((SM.K8,), False, True, True) in seen) and (((SM.K8,), False, False, False) in seen) and (((SM.K8, SM.REDUCE), True, True, False) in seen)


def query_of(c):
    """A GEMM-family row of small_ref.CASES as the arguments of the query: M, N, K, ta, tb, fuse, ws_bytes, align."""
    a = c.args
    align = 7 & ~(1 if a["shift"] in ("A", "M") else 0) & ~(2 if a["shift"] == "B" else 0)
    if c.entry == "sgx_gemm_f32":
        need = SM.gemm_ws_bytes(a["M"], a["N"], a["K"])
        return a["M"], a["N"], a["K"], a["ta"], a["tb"], 0, {"full": need, "null": 0, "short": need - 4}[a["ws"]], align
    if c.entry == "sgx_linear_fwd":
        return a["B"], a["N"], a["K"], 0, 1, 2 if a["bias"] or a["act"] else 0, 0, align
    if c.entry == "sgx_linear_bwd_data":
        return a["B"], a["K"], a["N"], 0, 0, 1 if a["mask"] else 0, 0, align
    return a["N"], a["K"], a["B"], 1, 0, (1 if a["mask"] else 0) | (2 if a["db"] else 0), 0, align


def test_every_gemm_row_gets_its_kernel_list_from_the_query(lib):
    rows = [c for c in SM.CASES if c.entry in ("sgx_gemm_f32", "sgx_linear_fwd", "sgx_linear_bwd_data", "sgx_linear_bwd_param")]
    assert len(rows) == sum(SM.ROWS[e] for e in ("sgx_gemm_f32", "sgx_linear_fwd", "sgx_linear_bwd_data", "sgx_linear_bwd_param"))
    for c in rows:
        q = query_of(c)
        got = lib_plan(lib, *q)
        assert (KINDS[got[0]],) + ((SM.REDUCE,) if got[1] > 1 else ()) == c.kernels, (c.id, got)
        assert got == SM.gemm_plan_ints(SM.gemm_plan_of(c), q[7]), (c.id, got)
        launches = [((got[2], got[3], got[4]), (256, 1, 1), 0)] + ([((got[5], 1, 1), (256, 1, 1), 0)] if got[1] > 1 else [])
        assert launches == SM.plan(c)[1], (c.id, got)                  # ... the geometry tests/test_gpu_small_paths.py holds the profiler's records to
    assert {query_of(c)[7] for c in rows} == {7, 6, 5}                 # an operand 4 bytes off on either side is among them


@pytest.mark.parametrize("M,N,K", [(0, 16, 16), (4, -1, 16), (4, 16, 0), (-3, -3, -3)])
def test_a_shape_that_is_not_positive_is_einval(lib, M, N, K):
    out = (ctypes.c_int * PLAN_INTS)()
    lib.sgx_clear_error()
    rc = lib.sgx_gemm_plan(M, N, K, 0, 0, 0, 0, 7, ctypes.addressof(out))
    msg = lib.sgx_last_error().decode(errors="replace")
    lib.sgx_clear_error()
    assert rc == SM.EINVAL and "gemm: bad shape" in msg and list(out) == [0] * PLAN_INTS, (rc, msg, list(out))


def test_a_null_output_is_einval(lib):
    assert lib.sgx_gemm_plan(4, 16, 16, 0, 0, 0, 0, 7, None) == SM.EINVAL
    lib.sgx_clear_error()
