"""Runs every row of the streaming kernels' GPU tests through native.lib() in one process and reports what each launched and wrote:
``python tests/streaming_runner.py [--write-geometry]``.  The rows are those of streaming_ref.CASES (through the RUNNERS of
tests/test_gpu_streaming_kernels.py) and the C-ABI kernel rows of tests/test_gpu_channels.py that give launch() an expected kernel list.  One
JSON line per row: id, kernel ids, per-launch [grid, block, lds], sha256 of each output's bytes (the streaming_ref.Guarded buffers of the row,
in the order they were made).  The process stops at the first HIP error.  Without --write-geometry the launches are compared with
tests/golden/streaming_launch.json; with it the file is written from them.  Two runs of one source tree print the same lines: a launcher
refactor is checked by comparing the output before and after."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import streaming_ref as SR  # noqa: E402
import test_gpu_channels as TC  # noqa: E402
import test_gpu_streaming_kernels as T  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
LAUNCHES = {}                       # row id -> [[kernel id, gx, gy, gz, bx, by, bz, lds], ...]
OUTPUTS = {}                        # row id -> [Guarded, ...]
_pending = []                       # outputs made since the last launch


class Recorded(SR.Guarded):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        _pending.append(self)


def record(row, launches):
    LAUNCHES.setdefault(row, []).extend(launches)
    OUTPUTS.setdefault(row, []).extend(_pending)
    del _pending[:]


def digest(t):
    return hashlib.sha256(t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def report(row, recorded, ok=True, **more):
    """Print a row and forget its outputs -> did it pass (its launches are the fixture's, unless the fixture is being written)."""
    la = LAUNCHES.get(row, [])
    if recorded is not None and ok and recorded.get(row) != la:
        ok, more = False, {"error": f"launches differ from tests/golden/streaming_launch.json: {recorded.get(row)}"}
    out = {"id": row, "ok": ok, "kernels": [r[0] for r in la], "launches": [[r[1:4], r[4:7], r[7]] for r in la],
           "sha256": [digest(g.t) for g in OUTPUTS.pop(row, [])], **more}
    print(json.dumps(out), flush=True)
    return ok


# the parametrisations of the three kernel-row tests of tests/test_gpu_channels.py
CHANNEL_ROWS = ([(TC.test_img_in_rows, J, dt) for J in (1, 2, 4, 8) for dt in (F32, BF16)]
                + [(TC.test_img_out_rows, J, dt) for J in (1, 2, 4) for dt in (F32, BF16)]
                + [(TC.test_img_wgrad_rows, J, dt) for J in (1, 2, 4, 8) for dt in (F32, BF16)])


def groups():
    """(name, the call that runs its rows): one row of CASES, or one parametrisation of a channels test with a row per call of launch()."""
    N = T._native()
    for c in SR.CASES:
        yield c.id, (lambda c=c: T.RUNNERS[c.entry](N.lib(), N, c))
    for fn, J, dt in CHANNEL_ROWS:
        yield f"{fn.__name__}[{J}-{SR.tname(dt)}]", (lambda fn=fn, J=J, dt=dt: fn(J, dt))


def main(write):
    SR.RECORDER, SR.Guarded = record, Recorded
    recorded = None
    if not write:
        with open(SR.GEOMETRY_PATH) as f:
            recorded = json.load(f)
    bad = 0
    for name, call in groups():
        before = set(LAUNCHES)
        err = None
        try:
            call()
            torch.cuda.synchronize()
        except AssertionError as e:
            err = str(e)[:600]
        except RuntimeError as e:                            # a HIP error: stop here
            print(json.dumps({"id": name, "ok": False, "error": "HIP: " + str(e)[:600]}), flush=True)
            return 3
        rows = [r for r in LAUNCHES if r not in before]
        if rows and _pending:                                # outputs made after the group's last launch (a second call that is compared with the first)
            OUTPUTS[rows[-1]].extend(_pending)
        del _pending[:]
        for r in rows:
            bad += not report(r, recorded, err is None, **({"error": err} if err else {}))
        if not rows:
            bad += 1
            print(json.dumps({"id": name, "ok": False, "error": err or "no launch"}), flush=True)
        if T._FAULT is not None:
            return 3
    if write and not bad:
        with open(SR.GEOMETRY_PATH, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in LAUNCHES.items()) + "\n}\n")
    if recorded is not None and set(recorded) != set(LAUNCHES):
        print(json.dumps({"id": "fixture", "ok": False, "error": f"rows not run: {sorted(set(recorded) - set(LAUNCHES))[:20]}"}), flush=True)
        bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main("--write-geometry" in sys.argv[1:]))
