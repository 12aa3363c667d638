#!/usr/bin/env python3
"""The record behind tests/test_gepi_plan.py (b): what sgx_gepi_ws_bytes(B, HW, C) and sgx_blur3x3_stats_nparts(B, H, W, C, dtype) return over
that test's grid (H x W = HW as test_gepi_plan.hw_split factors it; C = 4 with fp32 only).

Recorded from the library of the commit BEFORE the generator epilogue's launchers were folded into plans and its workspace into one view;
re-record only with a change that means to move the workspace layout or the blur's strip geometry, from the library that makes it, and read
the fixture's diff:

    python tests/golden/make_golden_gepi_ws.py          (needs no GPU; SGX_HIP_LIB=<path> records from another build of the library)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_gepi_plan as T  # noqa: E402

from stylegan.pytorch_amd import native  # noqa: E402


def main():
    if not os.environ.get("SGX_HIP_LIB"):
        native.build()
    # (not native.lib(): a library from before sgx_gepi_plan lacks that symbol; the two functions recorded here are all this needs)
    import ctypes
    L = ctypes.CDLL(native.LIB_PATH)
    L.sgx_gepi_ws_bytes.restype, L.sgx_gepi_ws_bytes.argtypes = native.SIGNATURES["sgx_gepi_ws_bytes"]
    L.sgx_blur3x3_stats_nparts.restype, L.sgx_blur3x3_stats_nparts.argtypes = native.SIGNATURES["sgx_blur3x3_stats_nparts"]
    ws, nparts = T.host_sizes(L)
    axes = {"B": list(T.BATCHES), "HW": list(T.PIXELS), "C": list(T.CHANNELS)}
    with open(T.FIXTURE, "w") as f:
        f.write('{"axes": %s,\n "ws_bytes": %s,\n "blur_nparts": %s}\n' % (json.dumps(axes), json.dumps(ws), json.dumps(nparts)))
    print("wrote %s: %d workspace sizes, %d partial counts from %s" % (T.FIXTURE, len(ws), len(nparts), native.LIB_PATH))


if __name__ == "__main__":
    main()
