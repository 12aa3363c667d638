"""The small-problem kernels of the batch-4 step alone on the GPU: microseconds per launch, and their outputs on fixed seeded inputs.

    python tools/small_probe.py --out DIR            time every case and save its outputs as DIR/<case>.npy
    python tools/small_probe.py --compare DIR_A DIR_B    compare two such directories bit for bit (no GPU)

``SGX_HIP_LIB=/path/to/other/libsgx_hip.so`` probes another build of the library (native.py reads it), so a change whose arithmetic
per output element is meant to stay what it was is checked by probing both builds and comparing.  Times are the mean of back-to-back
launches between two events (the launch floor of an empty kernel is about 6.5 us on this measure)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compare(a, b):
    names = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
    bad = 0
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        same = x.shape == y.shape and x.tobytes() == y.tobytes()
        if not same:
            bad += 1
            d = np.abs(x.astype(np.float64) - y.astype(np.float64)).max() if x.shape == y.shape else float("nan")
            print(f"DIFFERENT {f}: max abs difference {d:.3e}")
    print(f"{len(names) - bad} of {len(names)} arrays identical")
    return 1 if bad or not names else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=4)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))

    import torch

    from stylegan.pytorch_amd import functional as Fn
    from stylegan.pytorch_amd import native as N
    dev = torch.device("cuda:0")
    L = N.lib()
    B = a.batch
    gen = torch.Generator(device="cpu").manual_seed(1234)

    def rnd(*shape, dtype=torch.float32):
        return torch.randn(*shape, generator=gen).to(dtype).to(dev)

    results = []

    def run(name, launch, outs):
        launch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            launch()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000.0 / a.reps
        results.append((name, us))
        print(f"{name:40s} {us:8.2f} us", flush=True)
        if a.out:
            for i, o in enumerate(outs):
                np.save(os.path.join(a.out, f"{name.replace(' ', '_')}.{i}.npy"), o.detach().float().cpu().numpy())

    if a.out:
        os.makedirs(a.out, exist_ok=True)
    st = N.stream

    # ---- fp32 GEMM: (M, N, K, ta, tb) as the step calls sgx_gemm_f32 (discriminator head) ...
    for (M, Nn, K, ta, tb) in [(B, 512, 1, 0, 0), (512, 8192, B, 1, 0), (B, 512, 8192, 0, 1), (B, 8192, 512, 0, 0), (B, 1, 512, 0, 1),
                               (1, 512, B, 1, 0), (33, 64, 3, 1, 0), (33, 64, 2, 0, 0), (37, 50, 77, 0, 0), (37, 50, 77, 1, 1), (20, 33, 100, 1, 0), (20, 33, 100, 0, 1)]:
        A = rnd(K, M) if ta else rnd(M, K)
        Bm = rnd(Nn, K) if tb else rnd(K, Nn)
        C = torch.empty(M, Nn, device=dev)
        wsb = L.sgx_gemm_ws_bytes(M, Nn, K)
        ws = N.workspace(wsb, dev) if wsb else None
        run(f"gemm {M}x{Nn}x{K} t{ta}{tb}",
            lambda: N.check(L.sgx_gemm_f32(N.ptr(A), N.ptr(Bm), N.ptr(C), M, Nn, K, ta, tb, 0.37, N.ptr(ws), wsb, st()), "gemm"), [C])
    # ---- ... and the fused EqualizedLinear launches (mapping network: two passes of the batch in one call at batch 4)
    for (Bb, Nn, K) in [(2 * B, 512, 512), (5, 40, 24)]:
        x, w, bias, gy = rnd(Bb, K), rnd(Nn, K), rnd(Nn), rnd(Bb, Nn)
        y, gx, dw, db = torch.empty(Bb, Nn, device=dev), torch.empty(Bb, K, device=dev), torch.empty(Nn, K, device=dev), torch.empty(Nn, device=dev)
        run(f"linear_fwd {Bb}x{Nn}x{K}", lambda: N.check(L.sgx_linear_fwd(N.ptr(x), N.ptr(w), N.ptr(bias), N.ptr(y), Bb, Nn, K, 0.05, 0.01,
                                                                           N.ACT_LRELU, st()), "linear_fwd"), [y])
        run(f"linear_bwd_data {Bb}x{Nn}x{K}", lambda: N.check(L.sgx_linear_bwd_data(N.ptr(gy), N.ptr(y), N.ptr(w), N.ptr(gx), Bb, Nn, K, 0.05,
                                                                                     st()), "linear_bwd_data"), [gx])
        run(f"linear_bwd_param {Bb}x{Nn}x{K}", lambda: N.check(L.sgx_linear_bwd_param(N.ptr(gy), N.ptr(y), N.ptr(x), N.ptr(dw), N.ptr(db), Bb, Nn,
                                                                                       K, 0.05, 0.01, st()), "linear_bwd_param"), [dw, db])
    # ---- minibatch stddev at the discriminator's 4x4 top
    for dtype in (torch.bfloat16, torch.float32):
        for (Bb, HW, Cc, Cpad) in [(B, 16, 512, 544), (8, 16, 24, 32), (2, 16, 16, 32)]:
            x, ggx = rnd(Bb, HW, Cc, dtype=dtype), rnd(Bb, HW, Cc, dtype=dtype)
            dy = rnd(Bb, HW, Cpad, dtype=dtype)
            y, ddy = torch.empty_like(dy), torch.empty_like(dy)
            dx, gx = torch.empty_like(x), torch.empty_like(x)
            tag = f"B{Bb} C{Cc} {'bf16' if dtype == torch.bfloat16 else 'f32'}"
            run(f"mbstd_fwd {tag}", lambda: N.check(L.sgx_mbstd_fwd(N.ptr(x), N.ptr(y), Bb, HW, Cc, Cpad, N.dt(x), st()), "mbstd_fwd"), [y])
            run(f"mbstd_bwd {tag}", lambda: N.check(L.sgx_mbstd_bwd(N.ptr(dy), N.ptr(x), N.ptr(dx), Bb, HW, Cc, Cpad, N.dt(x), st()), "mbstd_bwd"), [dx])
            run(f"mbstd_bwd2 {tag}", lambda: N.check(L.sgx_mbstd_bwd2(N.ptr(ggx), N.ptr(dy), N.ptr(x), N.ptr(ddy), N.ptr(gx), Bb, HW, Cc, Cpad,
                                                                      N.dt(x), st()), "mbstd_bwd2"), [ddy, gx])
    # ---- the 18 style affines of the 1024x1024 generator in one launch (and a ragged small set)
    for (Bb, D, ns) in [(B, 512, [1024] * 10 + [512] * 2 + [256] * 2 + [128] * 2 + [64] * 2), (3, 64, [40, 24, 100]), (32, 128, [72, 200])]:
        G = len(ns)
        ws_, bs_ = [rnd(n, D) for n in ns], [rnd(n) for n in ns]
        lm = rnd(G, Bb, D)
        meta = tuple((g, 0.04 + 0.001 * g, 1.0) for g in range(G))
        lm_r = lm.clone().requires_grad_(True)
        params = [t.requires_grad_(True) for t in ws_ + bs_]
        ys = Fn.GroupedStyleFn.apply(lm_r, meta, *params)
        ent = next(v for k, v in Fn._STYLE_TABLES.items() if k[0] == tuple(w.data_ptr() for w in ws_))
        table, ns_, yoffs, ytotal, tiles = ent
        y = torch.empty(ytotal, device=dev)
        gy = rnd(ytotal)
        glm = torch.empty_like(lm)
        dw, db = torch.empty(sum(ns), D, device=dev), torch.empty(sum(ns), device=dev)
        tag = f"G{G} B{Bb} D{D}"
        run(f"style_fwd {tag}", lambda: N.check(L.sgx_style_fwd(N.ptr(lm), N.ptr(table), N.ptr(y), G, Bb, D, tiles, st()), "style_fwd"), [y])
        run(f"style_bwd_data {tag}", lambda: N.check(L.sgx_style_bwd_data(N.ptr(gy), N.ptr(table), N.ptr(glm), G, Bb, D, max(ns), st()),
                                                     "style_bwd_data"), [glm])
        run(f"style_bwd_param {tag}", lambda: N.check(L.sgx_style_bwd_param(N.ptr(gy), N.ptr(lm), N.ptr(table), N.ptr(dw), N.ptr(db), G, Bb, D,
                                                                            tiles, st()), "style_bwd_param"), [dw, db])
        del ys


if __name__ == "__main__":
    main()
