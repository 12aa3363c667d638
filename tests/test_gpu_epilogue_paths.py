"""-m gpu: every launch path of the generator layer epilogue (csrc/gepi.hip) at the C ABI, under the decoupled per-element criterion of
tests/epilogue_ref.py.  Rows of the default environment run in this process, one test per row; the rows behind process-wide switches run in
one fresh child process per group (tests/epilogue_runner.py), whose y / dx must equal the default rows' bit for bit where gepi.hip promises
that (gepi_apply1 = gepi_apply, gepi_bwd2s = gepi_pass<T, 2>, nontemporal = plain, separate finalize = folded)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import epilogue_ref as ER
import epilogue_runner as RUN
import streaming_ref as SR

pytestmark = pytest.mark.gpu

DEFAULT = [c for c in ER.CASES if c.group == "default"]
CHILD_TIMEOUT = 300                 # seconds; a group takes a few
_CHILD_DEAD = None


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", DEFAULT, ids=[c.id for c in DEFAULT])
def test_epilogue_case(case):
    assert all(os.environ.get(k) is None for g in ER.GROUPS.values() for k in g), "the default rows need the default switches"
    res = RUN.run_case(case)
    print(case.id, {k: (f"{v:.3f}" if isinstance(v, float) else v) for k, v in res.items() if k != "hash"})


@pytest.mark.parametrize("group", [g for g in ER.GROUPS if g != "default"])
def test_epilogue_group_in_a_fresh_process(group):
    """The switches are read once per process: the group's rows run in a child with the environment added.  After a child that ended by a
    signal, a timeout or a HIP error (any exit status but 0: failing rows alone leave it 0) no further child is started, and nothing more
    runs on the device from this process either."""
    global _CHILD_DEAD
    assert _CHILD_DEAD is None, f"not run: {_CHILD_DEAD}"
    assert RUN._FAULT is None, f"not run: the GPU reported an error in an earlier case ({RUN._FAULT})"
    rows = [c for c in ER.CASES if c.group == group]
    env = dict(os.environ, **ER.GROUPS[group])
    try:
        r = subprocess.run([sys.executable, RUN.__file__, group], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        RUN._FAULT = _CHILD_DEAD = f"the child of group {group} ran past {CHILD_TIMEOUT} s"
        raise AssertionError(_CHILD_DEAD)
    if r.returncode != 0:
        RUN._FAULT = _CHILD_DEAD = f"the child of group {group} ended by signal {-r.returncode}" if r.returncode < 0 else f"the child of group {group} stopped with exit status {r.returncode}"
    out = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    bad = [o for o in out if not o["ok"]]
    assert r.returncode == 0 and not bad, f"group {group}: exit status {r.returncode}; {bad[:3]}\n{r.stderr[-2000:]}"
    assert [o["id"] for o in out] == [c.id for c in rows], "every row of the group reported"
    for c, o in zip(rows, out):
        print(c.id, {k: (f"{v:.3f}" if isinstance(v, float) else v) for k, v in o.items() if k not in ("hash", "id", "ok")})
        twin = c.args.get("twin")
        if twin:
            assert o["hash"] == RUN.run_case(ER.BY_ID[twin])["hash"], f"{c.id}: the bits differ from the default row {twin} ({c.why})"
    assert sum(1 for c in rows if c.args.get("twin")) >= 2


@pytest.mark.parametrize("rej", ER.REJECTIONS, ids=[r[0] for r in ER.REJECTIONS])
def test_gepi_check_rejections_launch_nothing(rej):
    """Arguments gepi_check refuses, in all three entry points: the documented code comes back, no kernel is launched, nothing is written."""
    N = RUN.native(); L = N.lib()
    rid, B, HW, C, dt, short, code, why = rej
    with RUN.sticky(rid):
        _rejection(N, L, rid, B, HW, C, short, code, why)


def _rejection(N, L, rid, B, HW, C, short, code, why):
    x = torch.zeros(B * HW * 64, device=RUN.DEV)
    v = torch.zeros(4096, device=RUN.DEV)
    out = SR.Guarded((B * HW * 64,), torch.float32, RUN.DEV)
    wsb = max(L.sgx_gepi_ws_bytes(B, HW, 32), L.sgx_gepi_ws_bytes(B, HW, C)) if not short else L.sgx_gepi_ws_bytes(B, HW, C) - short
    ws = N.workspace(wsb + 16, RUN.DEV)
    p, st = RUN.p, N.stream()
    for entry, call in (("sgx_gepi_fwd", lambda: L.sgx_gepi_fwd(p(x), None, p(v), p(v), p(v), p(out.t), p(out.t), p(out.t), p(ws), wsb, None, 0, B, HW, C, 3, 0, st)),
                        ("sgx_gepi_stats", lambda: L.sgx_gepi_stats(p(x), None, p(v), p(v), p(out.t), p(out.t), p(ws), wsb, None, 0, B, HW, C, 3, 0, st)),
                        ("sgx_gepi_bwd", lambda: L.sgx_gepi_bwd(p(x), p(x), None, p(v), p(v), p(v), p(v), p(v), p(out.t), p(out.t), p(out.t), None, p(ws), wsb, B, HW, C, 3, 0, st))):
        N.prof_start(1)
        try:
            rc = call()
            torch.cuda.synchronize()
        finally:
            N.prof_start(0)
        assert rc == code, f"{rid} {entry} ({why}): returned {rc}, documented {code}"
        assert N.prof_records() == [], f"{rid} {entry}: a kernel was launched"
        assert L.sgx_last_error(), rid
        L.sgx_clear_error()
    assert bool((out.buf == SR.SENTINEL).all()), f"{rid}: an output was written"
