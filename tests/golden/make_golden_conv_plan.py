#!/usr/bin/env python3
"""The record behind tests/test_conv_plan.py: what the host-side plan queries of libsgx_hip.so answer for every shape of that test's grid
(tile slots of the fused-statistics convolution, which fused variants exist, the split-K workspace, the first-generation tile
configuration of the three geometries), all bf16, at 256 compute units.

Recorded from the library of the commit BEFORE the convolution launchers were folded into one dispatch table and one grid plan; re-record
only with a change that means to move a launch decision, from the library that makes it, and read the fixture's diff:

    python tests/golden/make_golden_conv_plan.py          (needs no GPU; SGX_HIP_LIB=<path> records from another build of the library)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_conv_plan as T  # noqa: E402

from stylegan.pytorch_amd import native  # noqa: E402


def main():
    if not os.environ.get("SGX_HIP_LIB"):
        native.build()
    L = native.lib()
    rows = {T.key(s): T.record(L, s) for s in T.shapes()}
    with open(T.FIXTURE, "w") as f:
        f.write('{"ncu": 256, "columns": %s, "rows": {\n' % json.dumps(list(T.COLUMNS)))
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in rows.items()))
        f.write("\n}}\n")
    print("wrote %s: %d shapes from %s" % (T.FIXTURE, len(rows), native.LIB_PATH))


if __name__ == "__main__":
    main()
