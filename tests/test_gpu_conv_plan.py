"""-m gpu: the kernel that each default bf16 convolution entry point launches, on the smallest shapes that sit on either side of every rule
of the launch layer (csrc/conv2.hip conv2_pick, the entry points' own rules, csrc/conv.hip pick_cfg / conv_splitk_plan).  Each row calls
the entry point under the library's per-launch profiler and asserts the ordered list of (instantiation, description) -- literals, a record of
what the library launched before its launchers were folded into one dispatch table and one grid plan -- and that the NaN-prefilled output
holds no NaN afterwards.  What the kernels compute is covered by test_gpu_kernels.py / test_gpu_fusions.py; tests/test_conv_plan.py covers
the host-only plan queries on a wide grid.  The expectations are for the whole chip (256 compute units)."""
import pytest
import torch

from epilogue_runner import DEV, native, p, rnd, sticky
from wgrad_runner import profiled

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
K2, K3 = "conv2_kernel<%s>", "conv3_kernel<%s>"
G1 = "conv_kernel<bf16_t, %s>"

# (entry, B, H, W, Cin, Cout, [(kernel, description)], the rule)
ROWS = [
    ("conv3x3", 4, 128, 128, 128, 128, [(K2 % "0, 8, 2, 32, false, 0", "convS B4 128x128 128->128")], "8-wave 64-channel tiles fill the chip exactly (256 blocks)"),
    ("conv3x3", 3, 128, 128, 128, 128, [(K2 % "0, 8, 1, 32, false, 0", "convS B3 128x128 128->128")], "small grid: 8 waves x 32 channels"),
    ("conv3x3", 4, 64, 64, 256, 256, [(K2 % "0, 8, 1, 32, false, 0", "convS B4 64x64 256->256")], "small grid: 8 waves x 32 channels"),
    ("conv3x3", 4, 32, 32, 512, 512, [(K2 % "0, 4, 1, 32, false, 0", "convS B4 32x32 512->512")], "small grid: 4 waves x 32 channels"),
    ("conv3x3", 4, 16, 32, 512, 512, [(G1 % "32, 0, 8, 16, 128, 1, false", "convS B4 16x32 512->512")], "no second-generation shape fills the chip"),
    ("conv3x3", 4, 256, 256, 64, 32, [(K2 % "0, 8, 1, 32, false, 0", "convS B4 256x256 64->32")], "32 output channels, 8-wave tiles fill the chip"),
    ("conv3x3", 1, 256, 256, 64, 32, [(K2 % "0, 4, 1, 32, false, 0", "convS B1 256x256 64->32")], "32 output channels, only the 4-wave tiles fill the chip"),
    ("conv3x3", 1, 512, 512, 16, 16, [(K2 % "0, 8, 1, 16, true, 0", "convS B1 512x512 16->16")], "16 channels: two 8-wave blocks per CU"),
    ("conv3x3", 1, 256, 256, 16, 16, [(K2 % "0, 4, 1, 16, true, 0", "convS B1 256x256 16->16")], "16 channels: 4-wave tiles"),
    ("conv3x3", 1, 128, 128, 16, 16, [(G1 % "16, 0, 4, 16, 64, 1, false", "convS B1 128x128 16->16")], "16 channels: fewer 4-wave tiles than CUs"),
    ("conv4x4s2_down", 4, 256, 256, 64, 128, [(K2 % "1, 8, 2, 32, false, 0", "convD B4 256x256 64->128")], "8-wave 64-channel tiles fill the chip"),
    ("conv4x4s2_down", 2, 256, 256, 64, 128, [(K2 % "1, 8, 1, 32, false, 0", "convD B2 256x256 64->128")], "small grid: 8 waves x 32 channels"),
    ("conv4x4s2_down", 4, 128, 128, 128, 256, [(K2 % "1, 8, 1, 32, false, 0", "convD B4 128x128 128->256")], "small grid: 8 waves x 32 channels"),
    ("conv4x4s2_down", 4, 128, 128, 64, 32, [(G1 % "32, 1, 4, 16, 64, 1, false", "convD B4 128x128 64->32")], "32-channel stride-2 blocks are not taken"),
    ("conv4x4s2_down", 1, 1024, 512, 16, 32, [(K2 % "1, 4, 1, 16, false, 0", "convD B1 1024x512 16->32")], "16 input channels: 4-wave tiles"),
    ("conv_splitk", 4, 16, 16, 512, 512, [(G1 % "32, 1, 8, 8, 64, 1, true", "convD/k4 B4 16x16 512->512"), ("conv_splitk_finish", "conv_splitk_finish 256x512")],
     "the stride-2 launch that leaves the chip idle: 4 ways"),
    ("conv4x4s2_up", 4, 128, 128, 64, 32, [(K2 % "2, 4, 1, 32, false, 0", "convU B4 128x128 64->32")], "transposed: 4-wave tiles"),
    ("conv4x4s2_up", 4, 64, 64, 128, 64, [(G1 % "32, 3, 8, 16, 128, 1, false", "convU B4 64x64 128->64")], "transposed: fewer 4-wave tiles than CUs"),
    ("conv4x4s2_up", 1, 256, 256, 32, 16, [(G1 % "32, 3, 8, 16, 128, 1, false", "convU B1 256x256 32->16")], "the 32->16 transposed layer needs the blur entry"),
    ("conv3x3_stats", 4, 64, 64, 256, 256, [(K2 % "0, 8, 1, 32, false, 1", "convS+stats B4 64x64 256->256")], "as conv3x3, statistics epilogue"),
    ("conv3x3_stats", 1, 256, 256, 16, 16, [(K2 % "0, 4, 1, 16, true, 1", "convS+stats B1 256x256 16->16")], "as conv3x3, statistics epilogue"),
    ("conv3x3_signbits", 4, 32, 32, 512, 512, [(K2 % "0, 4, 1, 32, false, 0", "convS+bits B4 32x32 512->512")], "as conv3x3"),
    ("conv4x4s2_up_blur", 1, 256, 256, 32, 16, [(K2 % "2, 4, 1, 32, true, 2", "convU+blur*mask B1 256x256 32->16")], "32->16 with the blur epilogue"),
    ("conv4x4s2_up_blur_bits", 1, 256, 256, 32, 16, [(K2 % "2, 4, 1, 32, true, 2", "convU+blur*bits B1 256x256 32->16")], "32->16 with the blur epilogue"),
    ("conv4x4s2_up_blur", 4, 128, 128, 64, 32, [(K2 % "2, 4, 1, 32, false, 2", "convU+blur*mask B4 128x128 64->32")], "as conv4x4s2_up, blur epilogue"),
    ("conv4x4s2_up_blur_bits", 4, 128, 128, 64, 32, [(K2 % "2, 4, 1, 32, false, 2", "convU+blur*bits B4 128x128 64->32")], "as conv4x4s2_up, blur epilogue"),
    ("conv4x4s2_down_fade", 4, 128, 128, 128, 256, [(K2 % "1, 8, 1, 32, false, 0", "convD+fade B4 128x128 128->256")], "as conv4x4s2_down"),
    ("conv4x4s2_down_fade_rgb", 4, 128, 128, 128, 256, [(K2 % "1, 8, 1, 32, false, 0", "convD+fade(rgb) B4 128x128 128->256")], "as conv4x4s2_down"),
    ("conv_upblur", 1, 512, 512, 32, 16, [(K3 % "0, 8, 2, 2, 2, 0, 1", "convU*blur B1 512x512 32->16")], "8-wave tiles fill the chip"),
    ("conv_upblur", 1, 128, 128, 32, 16, [(K3 % "0, 4, 2, 2, 2, 0, 1", "convU*blur B1 128x128 32->16")], "fewer 8-wave tiles than CUs"),
]


def run(L, N, entry, B, H, W, Cin, Cout):
    """-> (the call, the NaN-prefilled output)."""
    geo = 1 if "down" in entry or entry == "conv_splitk" else (2 if "up" in entry else 0)
    OH, OW = (H // 2, W // 2) if geo == 1 else ((2 * H, 2 * W) if geo == 2 else (H, W))
    taps = 9 if geo == 0 else 16
    x = rnd((B, H, W, Cin), BF, 1)
    w = rnd((80 if entry == "conv_upblur" else taps, Cout, Cin), BF, 2, 0.05)
    bias = rnd((Cout,), F32, 3)
    y = torch.full((B, OH, OW, Cout), float("nan"), dtype=BF, device=DEV)
    like_y = lambda seed: rnd((B, OH, OW, Cout), BF, seed)
    bits = torch.zeros((B, OH, OW, max(Cout // 8, 1)), dtype=torch.uint8, device=DEV)
    st, shape, keep = N.stream(), (B, H, W, Cin, Cout), []
    if entry == "conv3x3":
        call = lambda: L.sgx_conv3x3(p(x), p(w), p(bias), p(y), *shape, N.ACT_LRELU, None, N.BF16, st)
    elif entry == "conv4x4s2_down":
        call = lambda: L.sgx_conv4x4s2_down(p(x), p(w), p(bias), p(y), *shape, N.ACT_LRELU, N.BF16, st)
    elif entry == "conv4x4s2_up":
        call = lambda: L.sgx_conv4x4s2_up(p(x), p(w), p(y), *shape, N.BF16, st)
    elif entry == "conv_splitk":
        nb = L.sgx_conv_splitk_ws_bytes(1, *shape, N.BF16)
        assert nb != 0, "the shape does not split"
        ws = N.workspace(nb, DEV)
        call = lambda: L.sgx_conv_splitk(1, p(x), p(w), p(bias), p(y), None, *shape, N.ACT_LRELU, N.BF16, p(ws), nb, st)
    elif entry == "conv3x3_stats":
        npart = L.sgx_conv3x3_stats_nparts(*shape, N.BF16)
        assert npart > 0, "the shape has no fused statistics"
        part = torch.full((B, npart, Cout, 2), float("nan"), dtype=torch.float64, device=DEV)
        noise, nw = rnd((B, H * W), F32, 4), rnd((Cout,), F32, 5)
        call = lambda: L.sgx_conv3x3_stats(p(x), p(w), p(y), p(bias), p(noise), p(nw), p(part), part.numel() * 8, *shape, N.BF16, st)
        keep.append(part)
    elif entry == "conv3x3_signbits":
        assert L.sgx_conv3x3_signbits_ok(*shape, N.BF16) == 1
        call = lambda: L.sgx_conv3x3_signbits(p(x), p(w), p(bias), p(y), p(bits), *shape, N.ACT_LRELU, None, N.BF16, st)
    elif entry == "conv4x4s2_up_blur":
        assert L.sgx_conv4x4s2_up_blur_ok(*shape, N.BF16) == 1
        mask = like_y(6)
        call = lambda: L.sgx_conv4x4s2_up_blur(p(x), p(w), p(y), p(mask), *shape, N.BF16, st)
    elif entry == "conv4x4s2_up_blur_bits":
        call = lambda: L.sgx_conv4x4s2_up_blur_bits(p(x), p(w), p(y), p(bits), *shape, N.BF16, st)
    elif entry == "conv4x4s2_down_fade":
        assert L.sgx_conv4x4s2_down_fade_ok(*shape, N.BF16) == 1
        resid = like_y(7)
        call = lambda: L.sgx_conv4x4s2_down_fade(p(x), p(w), p(bias), p(resid), 0.75, 0.25, None, p(y), p(bits), *shape, N.BF16, st)
    elif entry == "conv4x4s2_down_fade_rgb":
        pimg, wr = rnd((B, OH, OW, 3), F32, 8), rnd((Cout, 3), F32, 9)
        call = lambda: L.sgx_conv4x4s2_down_fade_rgb(p(x), p(w), p(bias), p(pimg), p(wr), 0.5, None, 1.0, 1.0, 0.75, 0.25, None, p(y), p(bits), *shape, N.BF16, st)
    else:
        assert entry == "conv_upblur" and L.sgx_conv_upblur_ok(*shape, N.BF16) == 1
        call = lambda: L.sgx_conv_upblur(p(x), p(w), p(y), None, *shape, N.BF16, st)
    return call, [y] + keep


@pytest.mark.parametrize("row", ROWS, ids=["%s-B%d-%dx%d-%d-%d" % r[:6] for r in ROWS])
def test_default_path_launches_the_recorded_kernel(row):
    entry, B, H, W, Cin, Cout, want, why = row
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    if ncu != 256:
        pytest.skip(f"the expectations are for 256 compute units, this device has {ncu}")
    N = native()
    with sticky("%s B%d %dx%d %d->%d" % row[:6]):            # (after a HIP error nothing more is started on the device)
        call, outs = run(N.lib(), N, entry, B, H, W, Cin, Cout)
        rc, ran = profiled(entry, call)
        print(entry, (B, H, W, Cin, Cout), rc, ran)
        N.check(rc, "sgx_" + entry)
        assert ran == want, f"launched {ran}, recorded {want} ({why})"
        for t in outs:
            assert not bool(torch.isnan(t).any()), "an element of the output was not written"
