#!/usr/bin/env python3
"""The record behind tests/test_wgrad_plan.py (c): what sgx_wgrad_ws_bytes returns for every shape of that test's grid, at 256 compute units.

Recorded from the library of the commit BEFORE the weight-gradient launchers were folded into one plan; re-record only with a change that
means to move the workspace size, from the library that makes it, and read the fixture's diff:

    python tests/golden/make_golden_wgrad_ws.py          (needs no GPU; SGX_HIP_LIB=<path> records from another build of the library)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_wgrad_plan as T  # noqa: E402

from stylegan.pytorch_amd import native  # noqa: E402


def main():
    if not os.environ.get("SGX_HIP_LIB"):
        native.build()
    L = native.lib()
    axes = {"taps": list(T.TAPS), "B": list(T.BATCHES), "H": list(T.HEIGHTS), "Ck": list(T.CHANNELS), "Cn": list(T.CHANNELS)}
    sizes = [L.sgx_wgrad_ws_bytes(*s) for s in T.shapes()]
    with open(T.FIXTURE, "w") as f:
        f.write('{"ncu": %d, "axes": %s,\n "ws_bytes": %s}\n' % (T.NCU, json.dumps(axes), json.dumps(sizes)))
    print("wrote %s: %d shapes from %s" % (T.FIXTURE, len(sizes), native.LIB_PATH))


if __name__ == "__main__":
    main()
