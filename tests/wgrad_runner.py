"""Runs rows of wgrad_ref.CASES through native.lib() on the GPU: in-process for tests/test_gpu_wgrad_paths.py, and as a fresh child process for
the rows that need process-wide switches (``python wgrad_runner.py GROUP`` with the group's environment: one JSON line per row, the process
stops at the first HIP error).  Each row: the library's profiler brackets the call, the kernels that ran must be exactly the row's and the
finishing launch must report the restated split count, dW / db / the workspace sit in streaming_ref.Guarded buffers (the workspace exactly as
large as the row says, sentinel-filled: a partial that is read without having been written is a NaN), and the values meet wgrad_ref's
criteria: bit equality on integer rows, the chain bound on the others.  Before the call the row's shape and workspace are put to sgx_wgrad_plan:
the generation, the finishing launch's ``ns`` and the pre-reduction it announces must be what the profiler then shows, and so must the split
count where the finish note carries it (no pre-reduction); behind a pre-reduction the note shows the groups, and the split count is compared
with the restated one the row pins."""
import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import epilogue_runner as ERUN  # noqa: E402
import streaming_ref as SR  # noqa: E402
import wgrad_ref as WR  # noqa: E402
from epilogue_runner import DEV, digest, ints, native, p, rnd, sticky  # noqa: E402

F32 = torch.float32
RESULTS = {}                        # row id -> what run_case returned (ratios, hash): rows run once per process


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def operand(shape, dtype, seed, data):
    if data == "int":
        return ints(shape, dtype, seed)
    t = rnd(shape, F32, seed)
    return (t.abs() if data == "abs" else t).to(dtype)


def family(kernels):
    k = kernels[0]
    fam = "wgrad16_s" if k.startswith("wgrad16") else "wgrad2_s" if k.startswith("wgrad2_s") else "wgrad2_d" if k.startswith("wgrad2_d") else \
        "gen1_bf16" if "bf16_t" in k else "gen1_f32"
    return fam + ("+pre" if WR.PRE in kernels else "")


def profiled(what, call):
    """The call under the library's profiler -> (its return code, [(kernel_id, description)] of every launch in order)."""
    N = native()
    with sticky(what):
        N.prof_start(1)
        try:
            rc = call()
            torch.cuda.synchronize()
        finally:
            N.prof_start(0)
        return rc, [(SR.kernel_id(r[0]), r[4]) for r in N.prof_records()]


def run(L, N, c):
    a = c.args
    B, Hh, W, Ck, Cn, O, I, mode, acc = a["B"], a["H"], a["W"], a["Ck"], a["Cn"], a["O"], a["I"], a["mode"], a["acc"]
    cus = ncu()
    geo, taps = (0, 9) if mode == "S" else (1, 16)
    Hn, Wn = Hh // (geo + 1), W // (geo + 1)
    env = WR.group_env(c.group)
    wsq = L.sgx_wgrad_ws_bytes(taps, B, Hh, W, Ck, Cn)
    assert wsq == WR.ws_bytes(taps, B, Hh, W, Ck, Cn, env, cus), f"{c.id}: sgx_wgrad_ws_bytes returns {wsq}, restated {WR.ws_bytes(taps, B, Hh, W, Ck, Cn, env, cus)}"
    wsb = WR.row_ws(c, cus)
    pl = WR.row_plan(c, cus, wsb)
    want_ns = WR.NS_AT_304.get(c.id, a["ns"]) if cus == 304 else a["ns"]
    assert (pl.kernels, pl.nsplit) == (c.kernels, want_ns), \
        f"{c.id}: at {cus} CUs the restated rules give {pl.kernels} with {pl.nsplit} splits, the row expects {c.kernels} with {want_ns}"
    xk, xn = operand((B, Hh, W, Ck), c.dtype, 200, a["data"]), operand((B, Hn, Wn, Cn), c.dtype, 201, a["data"])
    dW0, db0 = ints((O, I, 3, 3), F32, 202) * 16.0, ints((O,), F32, 203) * 16.0                # |prefill| <= 48
    dW, db, ws = SR.Guarded((O, I, 3, 3), F32, DEV), (SR.Guarded((O,), F32, DEV) if a["bias"] else None), SR.Guarded((max(wsb, 16),), torch.uint8, DEV)
    if acc & 1:
        dW.t.copy_(dW0)
    if db is not None and acc & 2:
        db.t.copy_(db0)
    scale = WR.scale_of(c)
    dtc = 0 if c.dtype == F32 else 1
    if geo == 0:
        call = lambda: L.sgx_wgrad3x3_param(p(xk), p(xn), p(dW.t), p(db.t if db else None), p(ws.t), wsb, B, Hh, W, Ck, Cn, a["adjoint"], scale, O, I, acc, dtc, N.stream())
    else:
        call = lambda: L.sgx_wgrad4x4s2_param(p(xk), p(xn), p(dW.t), p(db.t if db else None), p(ws.t), wsb, B, Hh, W, Ck, Cn, WR.MODES[mode], scale, O, I, acc, dtc, N.stream())
    said = (ctypes.c_int * 11)()
    said_rc = L.sgx_wgrad_plan(taps, B, Hh, W, Ck, Cn, dtc, wsb, ctypes.addressof(said))
    if said_rc:
        L.sgx_clear_error()
    rc, recs = profiled(c.id, call)
    ran = tuple(k for k, _ in recs)
    assert said_rc == rc, f"{c.id}: sgx_wgrad_plan returned {said_rc}, the call {rc}"
    assert rc == pl.rc == a["rc"], f"{c.id}: returned {rc} ({L.sgx_last_error().decode(errors='replace')}), expected {a['rc']}"
    assert ran == pl.kernels, f"{c.id}: launched {ran}, expected {pl.kernels} ({c.why})"
    for g, what in ((dW, "dW"), (db, "db"), (ws, "workspace")):
        if g is not None:
            g.assert_intact(f"{c.id} {what}")
    res = {"family": family(pl.kernels) if pl.kernels else "none", "ns": pl.nsplit}
    if rc:                                                                                    # an error return before any launch: nothing written
        L.sgx_clear_error()
        for g, what in ((dW, "dW"), (db, "db"), (ws, "workspace")):
            assert g is None or bool((g.buf == SR.SENTINEL).all()), f"{c.id}: {what} was written by a call that returned {rc}"
        return res
    fins = [d for k, d in recs if k.startswith("wgrad_finish_kernel")]
    got_ns = int(re.search(r"ns(\d+)$", fins[0]).group(1)) if fins else None
    assert got_ns == pl.finish_ns, f"{c.id}: the finishing launch reports ns {got_ns} ({fins}), restated {pl.finish_ns}"
    seen = (1 if ran[0].startswith("wgrad_kernel<") else 2, pl.nsplit if WR.PRE in ran else (got_ns or 1), got_ns or 0, int(WR.PRE in ran))
    assert (said[0], said[7], said[8], said[9]) == seen, f"{c.id}: sgx_wgrad_plan says (generation, nsplit, finishing ns, pre-reduction) = {(said[0], said[7], said[8], said[9])}, the launches show {seen}"
    ref, S, rb, Sb = WR.wgrad(xk.double(), xn.double(), mode, SR.f32(scale), I, a["adjoint"], acc, dW0.double(), db0.double(), db is not None)
    if a["data"] == "int":
        assert WR.exact_ok(c) and torch.equal(ref.float().double(), ref), c.id
        nbad = int((dW.t != ref.float()).sum())
        assert torch.equal(dW.t.view(torch.int32), ref.float().view(torch.int32)), f"{c.id}: dW of an integer row differs from the exact value in {nbad} of {ref.numel()} places, first at {tuple(int(v) for v in (dW.t != ref.float()).nonzero()[0]) if nbad else '(signed zero)'}"
        if db is not None:
            assert torch.equal(db.t.view(torch.int32), rb.float().view(torch.int32)), f"{c.id}: db of an integer row differs from the exact value in {int((db.t != rb.float()).sum())} places"
        res["hash"] = digest(dW.t, *([db.t] if db is not None else []))
    else:
        res["dW"] = SR.assert_elementwise(dW.t, ref, S, pl.L, F32, f"{c.id} dW")
        if db is not None:
            res["db"] = SR.assert_elementwise(db.t, rb, Sb, pl.L, F32, f"{c.id} db")
    twin = a["twin"]
    if twin and WR.BY_ID[twin].group == c.group:                                              # (the parent compares across processes)
        assert res["hash"] == run_case(WR.BY_ID[twin])["hash"], f"{c.id}: the bits differ from the row {twin}"
    return res


def run_case(c):
    """Run a row once in this process (whose environment must be the row's group) -> its figures."""
    if c.id not in RESULTS:
        N = native()
        with sticky(c.id):                                   # the operands, the call and the fp64 references alike
            res = run(N.lib(), N, c)
        RESULTS[c.id] = res
        rep = os.environ.get("SGX_WGRAD_REPORT")             # a measuring run keeps every figure
        if rep:
            with open(rep, "a") as f:
                f.write(json.dumps({"id": c.id, **res}) + "\n")
    return RESULTS[c.id]


def main(group):
    for k in {k for g in WR.GROUPS.values() for k in g}:
        assert os.environ.get(k) == WR.GROUPS[group].get(k), f"{k} must be {WR.GROUPS[group].get(k)} for group {group}"
    for c in [c for c in WR.CASES if c.group == group]:
        try:
            print(json.dumps({"id": c.id, "ok": True, **run_case(c)}), flush=True)
        except AssertionError as e:
            print(json.dumps({"id": c.id, "ok": False, "error": str(e)[:600]}), flush=True)
            if ERUN._FAULT is not None:
                return 3
        except RuntimeError as e:                            # a HIP error: stop here
            print(json.dumps({"id": c.id, "ok": False, "error": "HIP: " + str(e)[:600]}), flush=True)
            return 3
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
