"""The shapes and calls of tests/test_gpu_kernels.py::test_one_load_blur_kernel_writes_the_bits_of_the_three_load_kernel, and their run in a
fresh process: ``python tests/blur_bits_child.py`` with SGX_BLUR_SHFL in the environment (the library reads it once per process) prints one
JSON line per shape and mode -- the sha256 of the output's bytes and the kernel that wrote it -- and stops at the first HIP error."""
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

DEV = "cuda:0"
# (tensors large enough for the streaming blur kernels: 8-row strips, >= 131072 strip lanes; heights that are not strip multiples)
SHAPES = [(torch.bfloat16, 6, 200, 512, 16), (torch.bfloat16, 10, 52, 256, 64), (torch.bfloat16, 16, 36, 128, 128),
          (torch.bfloat16, 6, 99, 448, 32), (torch.float32, 16, 72, 256, 16)]
# (the fourth had 3 images until the kernel names were asserted: 69888 strip lanes, the 2-row kernel whatever SGX_BLUR_SHFL says)
assert all(B * ((H + 7) // 8) * W * (C // (8 if dt == torch.bfloat16 else 4)) >= 131072 for dt, B, H, W, C in SHAPES)


def modes(dt):
    return [0, 1, 2, 4, 5] if dt == torch.bfloat16 else [0, 1, 2]


def run(dt, B, H, W, C):
    """-> x and {mode: (output, kernel id, sha256 of the output's bytes)} of one shape, each call under the library's profiler."""
    from stylegan.pytorch_amd import native as N
    L = N.lib()
    torch.manual_seed(C + H)
    x = torch.randn(B, H, W, C, device=DEV).to(dt)
    z = torch.randn(B, H, W, C, device=DEV).to(dt)
    bits = torch.randint(0, 256, (B, H, W, C // 8), device=DEV, dtype=torch.uint8)
    out = {}
    for mode in modes(dt):
        y = torch.full_like(x, 7.0)
        N.prof_start(1)
        try:
            if mode >= 4:
                rc = L.sgx_blur3x3_bits(N.ptr(x), N.ptr(bits), N.ptr(y), B, H, W, C, mode - 2, N.dt(x), N.stream())
            else:
                rc = L.sgx_blur3x3_act(N.ptr(x), N.ptr(z if mode == 2 else None), N.ptr(y), B, H, W, C, mode, N.dt(x), N.stream())
            torch.cuda.synchronize()
        finally:
            N.prof_start(0)
        N.check(rc, "blur")
        (rec,) = N.prof_records()
        sha = hashlib.sha256(y.reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()
        out[mode] = (y, SR.kernel_id(rec[0]), sha)
    return x, out


def main():
    for i, shape in enumerate(SHAPES):
        try:
            _, out = run(*shape)
        except RuntimeError as e:                            # a HIP error: stop here
            print(json.dumps({"shape": i, "error": str(e)[:600]}), flush=True)
            return 3
        for mode, (_, kernel, sha) in out.items():
            print(json.dumps({"shape": i, "mode": mode, "kernel": kernel, "sha256": sha}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
