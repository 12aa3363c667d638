"""-m gpu: the launch paths of the forward / data-gradient convolutions (the first half of csrc/conv.hip, csrc/conv2.hip) at the C ABI, per
element against the fp64 references of tests/conv_ref.py: bit equality on the integer rows, the chain bound on the randn / |randn| rows,
the exact kernel list and launch notes, guard bands and host queries on every row.  Rows of the default environment run in this process,
one test per row; the rows behind process-wide switches run in one fresh child process per group (tests/conv_runner.py), one after
another, and every switched integer row must give the bits of its default-environment twin: first generation = second, 4 waves = 8,
split-K = unsplit, bands on = off, nontemporal hints on = off, register store = LDS-transposed store, ...  The expectations are for 256 and
304 compute units."""
import json
import os
import subprocess
import sys

import pytest
import torch

import conv_ref as CR
import conv_runner as RUN
import epilogue_runner as ERUN

pytestmark = pytest.mark.gpu

DEFAULT = [c for c in CR.CASES if c.group == "default"]
CHILD_TIMEOUT = {g: 120 + 5 * sum(1 for c in CR.CASES if c.group == g) for g in CR.GROUPS}     # seconds; a row takes well under one
_CHILD_DEAD = None


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def show(id, res):
    print(id, {k: (f"{v:.3f}" if isinstance(v, float) else v) for k, v in res.items() if k not in ("hash", "id", "ok")})


def cu_count_or_skip():
    cus = RUN.ncu()
    if cus not in (256, 304):
        pytest.skip(f"the rows hold expectations for 256 and 304 compute units, this device has {cus}")


@pytest.mark.parametrize("case", DEFAULT, ids=[c.id for c in DEFAULT])
def test_conv_case(case):
    cu_count_or_skip()
    assert all(os.environ.get(k) is None for g in CR.GROUPS.values() for k in g), "the default rows need the default switches"
    show(case.id, RUN.run_case(case))
    torch.cuda.empty_cache()


@pytest.mark.parametrize("group", [g for g in CR.GROUPS if g != "default"])
def test_conv_group_in_a_fresh_process(group):
    """The switches are read once per process: the group's rows run in a child with the environment added.  After a child that ended by a
    signal, a timeout or a HIP error (any exit status but 0: failing rows alone leave it 0) no further child is started, and nothing more
    runs on the device from this process either."""
    global _CHILD_DEAD
    cu_count_or_skip()
    assert _CHILD_DEAD is None, f"not run: {_CHILD_DEAD}"
    assert ERUN._FAULT is None, f"not run: the GPU reported an error in an earlier case ({ERUN._FAULT})"
    rows = [c for c in CR.CASES if c.group == group]
    env = dict(os.environ, **CR.GROUPS[group])
    try:
        r = subprocess.run([sys.executable, RUN.__file__, group], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT[group])
    except subprocess.TimeoutExpired:
        ERUN._FAULT = _CHILD_DEAD = f"the child of group {group} ran past {CHILD_TIMEOUT[group]} s"
        raise AssertionError(_CHILD_DEAD)
    if r.returncode != 0:
        ERUN._FAULT = _CHILD_DEAD = f"the child of group {group} ended by signal {-r.returncode}" if r.returncode < 0 else f"the child of group {group} stopped with exit status {r.returncode}"
    out = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    bad = [o for o in out if not o["ok"]]
    assert r.returncode == 0 and not bad, f"group {group}: exit status {r.returncode}; {bad[:3]}\n{r.stderr[-2000:]}"
    assert [o["id"] for o in out] == [c.id for c in rows], "every row of the group reported"
    for c, o in zip(rows, out):
        show(c.id, o)
        twin = c.args["twin"]
        if twin:
            assert o["hash"] == RUN.run_case(CR.BY_ID[twin])["hash"], f"{c.id}: the bits differ from the default row {twin} ({c.why})"
    assert any(c.args["twin"] for c in rows) or all(c.args["rc"] for c in rows), group
