"""CPU: which kernel the default bf16 convolution path picks and how many tile slots it plans, per shape, against a record of the commit
before the launch layer of csrc/conv.hip / csrc/conv2.hip was folded into one dispatch table and one grid plan
(tests/golden/conv_plan.json, written by tests/golden/make_golden_conv_plan.py).  The plan queries are host-only: without a GPU the
library sizes its grids for 256 compute units, the MI355X's.  A row that differs is a changed launch decision: a deliberate one re-records
the fixture, and the diff of the fixture shows which shapes moved."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_plan.json")
BF16 = 1

BATCHES = (1, 2, 4, 8, 32)
HEIGHTS = (4, 8, 16, 17, 32, 64, 128, 256, 512, 1024)                     # W = H rounded up to a multiple of 32
CHANNELS = ((16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64), (96, 192), (128, 128), (128, 256), (256, 256), (256, 512),
            (512, 256), (512, 512))
MAX_ELEMS = 1 << 33
COLUMNS = ("stats_nparts", "signbits_ok", "down_fade_ok", "up_blur_ok", "upblur_ok", "splitk_ws_bytes", "config_s", "config_d", "config_u")


def shapes():
    for B in BATCHES:
        for H in HEIGHTS:
            W = (H + 31) // 32 * 32
            for Cin, Cout in CHANNELS:
                if B * H * W * max(Cin, Cout) <= MAX_ELEMS:
                    yield B, H, W, Cin, Cout


def record(L, shape):
    """The row of one shape: COLUMNS in order; None where the query does not apply (the stride-2 queries at odd H)."""
    B, H, W, Cin, Cout = shape
    even = H % 2 == 0
    cfg = []
    for geo in range(3):
        c5 = (ctypes.c_int * 5)()
        assert L.sgx_conv_config(geo, B, H, W, Cin, Cout, BF16, ctypes.addressof(c5)) == 0
        cfg.append(list(c5))
    return [L.sgx_conv3x3_stats_nparts(B, H, W, Cin, Cout, BF16),
            L.sgx_conv3x3_signbits_ok(B, H, W, Cin, Cout, BF16),
            L.sgx_conv4x4s2_down_fade_ok(B, H, W, Cin, Cout, BF16) if even else None,
            L.sgx_conv4x4s2_up_blur_ok(B, H, W, Cin, Cout, BF16),
            L.sgx_conv_upblur_ok(B, H, W, Cin, Cout, BF16),
            L.sgx_conv_splitk_ws_bytes(1, B, H, W, Cin, Cout, BF16) if even else None] + cfg


def key(shape):
    return "B%d %dx%d %d->%d" % shape


@pytest.fixture(scope="module")
def plan():
    from stylegan.pytorch_amd import native
    native.build()
    L = native.lib()
    return {key(s): record(L, s) for s in shapes()}


def test_the_grid_is_the_recorded_one():
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert fx["columns"] == list(COLUMNS) and fx["ncu"] == 256
    assert list(fx["rows"]) == [key(s) for s in shapes()] and len(fx["rows"]) == 697      # 3 of the 700 have a tensor above 2^33 elements


def test_spot_values(plan):
    col = {c: i for i, c in enumerate(COLUMNS)}
    assert plan["B4 32x32 512->512"][col["stats_nparts"]] == 16
    assert plan["B4 64x64 256->256"][col["stats_nparts"]] == 32
    assert plan["B4 1024x1024 16->16"][col["stats_nparts"]] == 512
    assert plan["B4 16x32 512->512"][col["splitk_ws_bytes"]] == 2097152
    assert plan["B4 512x512 32->16"][col["up_blur_ok"]] == 1 and plan["B4 512x512 32->16"][col["upblur_ok"]] == 1


def test_every_shape_plans_what_was_recorded(plan):
    with open(FIXTURE) as f:
        rows = json.load(f)["rows"]
    wrong = ["%s: %s" % (k, ", ".join("%s %s (recorded %s)" % (c, g, w) for c, g, w in zip(COLUMNS, plan[k], rows[k]) if g != w))
             for k in plan if plan[k] != rows[k]]
    assert not wrong, "%d of %d shapes plan differently:\n%s" % (len(wrong), len(plan), "\n".join(wrong[:40]))
