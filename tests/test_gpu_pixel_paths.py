"""-m gpu: every row of tests/pixel_ref.py on the kernels of csrc/diffaug.hip through the three C entries (sgx_diffaug, sgx_diffaug_gated,
sgx_diffaug_blit).  Per row: y in a guarded, sentinel-filled buffer at x's alignment; the partials workspace a guarded buffer of exactly
sgx_diffaug_ws_bytes bytes pre-filled with NaNs (afterwards: the slots of colour images finite, the slots of gated images without
the colour bit untouched, no NaN in y); the call under the library's profiler (what ran is what sgx_aug_plan reports, and is the
row's kernels); the exact elements bit for bit and every other element within the two-term bound of pixel_ref, the first offender
named; a second run with the same bits; a gated run equal to functional._diffaug with the same gates.  tests/test_pixel_coverage.py
holds the table to the launch sites and the criterion to an emulation and to planted errors, without a GPU."""
import collections

import numpy as np
import pytest
import torch

import ada_ref as A
import aug_ref as AR
import blit_ref as Bl
import pixel_ref as PR
import streaming_ref as SR
from gpu_util import DEV
from pixel_ref import BLIT, DIFFAUG, GATED

pytestmark = pytest.mark.gpu

ENTRY = {DIFFAUG: AR.DIFFAUG, GATED: AR.GATED, BLIT: AR.BLIT}
WORST, SEEN = collections.defaultdict(float), set()         # entry -> the worst err / bound of the rows run so far; their ids


def on_device(t, off):
    """A copy of the host array at a base ``off`` floats past a 16-byte boundary."""
    buf = torch.zeros(t.size + 4, device=DEV)
    v = buf[off:off + t.size].view(t.shape)
    v.copy_(torch.from_numpy(t).to(DEV))
    assert v.data_ptr() % 16 == 4 * off
    return v


def launch(entry, xd, ud, bitsd, policy, adjoint, with_bias, off, kernels):
    """One profiled call into guarded buffers -> (y, the workspace as fp32 [B][nparts]); guards, records and the plan checked."""
    from stylegan.pytorch_amd import native as N
    B, H, W, _ = xd.shape
    L = N.lib()
    nb = L.sgx_diffaug_ws_bytes(B, H, W)
    assert nb == 4 * B * PR.nparts(H, W)
    y = SR.Guarded((B, H, W, 3), torch.float32, DEV, shift=4 * off)
    ws = SR.Guarded((nb // 4,), torch.float32, DEV)
    assert y.t.data_ptr() % 16 == xd.data_ptr() % 16 == 4 * off and bool(torch.isnan(ws.t).all())
    N.prof_start(1)
    try:
        if entry == DIFFAUG:
            rc = L.sgx_diffaug(N.ptr(xd), N.ptr(y.t), N.ptr(ud), B, H, W, policy, adjoint, with_bias, N.ptr(ws.t), nb, N.stream())
        elif entry == GATED:
            rc = L.sgx_diffaug_gated(N.ptr(xd), N.ptr(y.t), N.ptr(ud), N.ptr(bitsd), B, H, W, policy, adjoint, with_bias, N.ptr(ws.t), nb, N.stream())
        else:
            rc = L.sgx_diffaug_blit(N.ptr(xd), N.ptr(y.t), ud.data_ptr(), ud.stride(0), None if bitsd is None else N.ptr(bitsd), B, H, W, policy, adjoint, with_bias,
                                    N.ptr(ws.t), nb, N.stream())
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    N.check(rc, entry)
    AR.assert_recorded_is_planned(N, ENTRY[entry], xd, y.t, policy, adjoint, with_bias)
    assert tuple(SR.kernel_id(r[0]) for r in N.prof_records()) == tuple(kernels), (N.prof_records(), kernels)
    y.assert_intact(entry + " y")
    ws.assert_intact(entry + " partials")
    return y.t, ws.t.view(B, -1)


def device_draws(c, u):
    """[B][7] for the three-op entries; [B][9] for the blit entry, alone or as the first columns of the rows of a [B][14] tensor."""
    if c.entry != BLIT:
        return torch.from_numpy(np.ascontiguousarray(u[:, :7])).to(DEV)
    if c.args["wide"]:
        wide = torch.rand(u.shape[0], 14, device=DEV)
        wide[:, :9] = torch.from_numpy(u).to(DEV)
        return wide[:, :9]
    return torch.from_numpy(u).to(DEV)


def run_controller(c):
    from stylegan.pytorch_amd import native as N
    L, B = N.lib(), c.args["B"]
    rng = np.random.default_rng(B)
    state = torch.from_numpy(A.new_state(0.5)).to(DEV)
    out = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    N.prof_start(1)
    try:
        if c.entry == "sgx_ada_gates":
            gu = rng.random((B, 3), dtype=np.float32)
            gu[0, 0], gu[1, 1] = 0.5, 0.0
            rc = L.sgx_ada_gates(N.ptr(torch.from_numpy(gu).to(DEV)), N.ptr(state), 7, N.ptr(out), B, N.stream())
            want = A.gates(gu, 0.5, 7)
        elif c.entry == "sgx_ada_gates_n":
            gu = rng.random((B, 5), dtype=np.float32)
            gu[0, 3], gu[1, 4] = 0.5, 0.0
            rc = L.sgx_ada_gates_n(N.ptr(torch.from_numpy(gu).to(DEV)), 5, 5, N.ptr(state), 31, N.ptr(out), B, N.stream())
            want = Bl.gates_n(gu, 0.5, 31)
        else:
            logits = rng.standard_normal(B).astype(np.float32)
            logits[0], logits[1] = np.float32(-0.0), np.float32(np.nan)
            adj = A.adjust_per_image(0.01)
            rc = L.sgx_ada_update(N.ptr(torch.from_numpy(logits).to(DEV)), B, N.ptr(state), 0.6, float(adj), 1, N.stream())
            want = A.controller(A.new_state(0.5), logits, 0.6, adj, 1)
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    N.check(rc, c.entry)
    assert tuple(SR.kernel_id(r[0]) for r in N.prof_records()) == c.kernels, N.prof_records()
    got = state.cpu().numpy() if c.entry == "sgx_ada_update" else out.cpu().numpy()
    assert np.array_equal(got.view(np.int32), np.asarray(want).view(np.int32)), (got, want)


@pytest.mark.parametrize("c", PR.CASES, ids=[c.id for c in PR.CASES])
def test_row(c):
    if c.entry in PR.CONTROLLER:
        return run_controller(c)
    from stylegan.pytorch_amd import functional as F
    a = c.args
    B, off, policy, adjoint, with_bias = a["B"], a["off"], a["policy"], a["adjoint"], a["with_bias"]
    x, u = PR.inputs(c)
    bits = PR.effective_bits(c)
    xd, ud = on_device(x, off), device_draws(c, u)
    bitsd = torch.tensor(bits, dtype=torch.int32, device=DEV) if a["gated"] else None
    y, part = launch(c.entry, xd, ud, bitsd, policy, adjoint, with_bias, off, c.kernels)
    # the partials: written for the colour images, and for nobody else
    for n, b in enumerate(bits):
        if b & 1:
            assert bool(torch.isfinite(part[n]).all()), (c.id, n, part[n])
        else:
            assert bool((part[n].view(torch.int32) == -1).all()), (c.id, n, "an image without the colour bit wrote its partials")
    assert bool(torch.isfinite(y).all()), c.id
    ref, exact, bound = PR.expected(c, x, u)
    r = PR.check(y.cpu().numpy(), ref, exact, bound, c.id)
    WORST[c.entry] = max(WORST[c.entry], r)
    SEEN.add(c.id)
    print(f"{c.id}: worst err / bound {r:.3f}")
    y2, _ = launch(c.entry, xd, ud, bitsd, policy, adjoint, with_bias, off, c.kernels)
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32)), (c.id, "two runs differ")
    if a["gated"]:
        uf = ud if c.entry != BLIT or policy & 24 else ud[:, :7].contiguous()      # without a blit bit the function takes seven draws (and the gated entry)
        assert torch.equal(y.view(torch.int32), F._diffaug(xd, uf, policy, adjoint, with_bias, bitsd).view(torch.int32)), (c.id, "functional._diffaug with the same gates")
        for n, b in enumerate(bits):
            if not b:
                assert torch.equal(y[n].view(torch.int32), xd[n].view(torch.int32)), (c.id, n, "bits 0: a copy")


# -0, +inf, -inf, quiet NaNs with payloads of either sign, a signalling NaN, the smallest denormals
SPECIAL = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc12345, 0xffc00001, 0x7f800123, 0x00000001, 0x80000001], np.uint32)


@pytest.mark.parametrize("entry,policy,N_,off", [(GATED, 7, 8, 0), (GATED, 7, 7, 0), (BLIT, 15, 8, 0), (BLIT, 31, 8, 1), (BLIT, 31, 8, 0), (BLIT, 31, 36, 0)],
                         ids=["apply4", "apply1", "row4", "row1", "tile-8", "tile-36"])
def test_gated_off_images_copy_special_values(entry, policy, N_, off):
    """Images with bits 0 beside augmented ones in one launch (the branch is per block): every word of theirs arrives as it is."""
    B, bits = 4, [0, policy, 0, policy]
    words = np.resize(SPECIAL, B * N_ * N_ * 3).view(np.float32).reshape(B, N_, N_, 3).copy()
    plain = PR.images(B, N_, N_, 3)
    words[1], words[3] = plain[1], plain[3]                                  # the augmented images hold ordinary numbers
    xd = on_device(words, off)
    u = PR.draws(8, N_, N_, 0, seed=1)[[1, 2, 5, 6]]
    ud = torch.from_numpy(u if entry == BLIT else np.ascontiguousarray(u[:, :7])).to(DEV)
    bitsd = torch.tensor(bits, dtype=torch.int32, device=DEV)
    for adjoint, with_bias in PR.MODES:
        y, _ = launch(entry, xd, ud, bitsd, policy, adjoint, with_bias, off, PR.kernels_of(entry, N_, N_, off, policy, adjoint))
        got, want = y.view(torch.int32).cpu(), xd.view(torch.int32).cpu()
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]), (adjoint, with_bias)
        assert not torch.equal(got[1], want[1]) and bool(torch.isfinite(y[1]).all()) and bool(torch.isfinite(y[3]).all())


def test_print_the_worst_ratios():
    """A record, not a check (every row asserts its own bound in PR.check): the worst err / bound per entry over the rows that ran before
    this in the same process -- all of them in a plain run of the file, fewer or none under -k or another order."""
    print(f"GPU, worst err / bound per entry over {'all' if len(SEEN) == len(PR.IMAGE_CASES) else len(SEEN)} image rows: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
