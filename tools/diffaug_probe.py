"""DiffAugment probe (csrc/diffaug.hip): what the augmentation costs on the MI355X.

  python tools/diffaug_probe.py --kernels [--batch 32 --res 1024]
      launches the forward (with bias) and the adjoint of policy color,translation,cutout a few times on one image batch; run it under
      ``rocprofv3 --kernel-trace --stats -d DIR -o diffaug -- python tools/diffaug_probe.py --kernels`` for per-kernel times.
  python tools/diffaug_probe.py --stats DIR/.../diffaug_kernel_stats.csv [--batch 32 --res 1024]
      per-kernel mean time from that run and the algorithmic bytes / time (sum pass: 12 B per pixel read; apply: 12 B read + 12 B written).
  python tools/diffaug_probe.py --ab [--batches 4,32 --repeats 4 --steps 8]
      step time at ffhq1024, bf16, hipGraph replay (bench.make_stylegan), policy off vs color,translation,cutout, interleaved on ONE
      StyleGAN object (each policy has its own captured graphs) -- prints one JSON line.
  python tools/diffaug_probe.py --ada-kernels [--batches 4,32 --res 1024 --iters 20]
      ADA's gated kernels against sgx_diffaug in one process (HIP events around ``iters`` back-to-back launches, best of 5): forward and
      adjoint with every image gated on (the same work as the ungated kernels), all off (copies) and every second image on; plus the
      gate and the controller launch -- prints one JSON line.
  python tools/diffaug_probe.py --ada-ab [--batches 4 --repeats 4 --steps 8]
      step time as in --ab, the policy alone vs ADA on top of it with p pinned to 1 (every image gated on: what ADA's own launches cost).
  python tools/diffaug_probe.py --blit-kernels [--batches 4,32 --res 1024 --iters 20]
      the pixel-blitting apply kernels against today's apply kernel on the same tensors, forward and adjoint, per launch from the
      library's own profiler (HIP events around every kernel; min and median over ``iters`` launches, variants interleaved): the row
      path with flips, the tile path with every k odd, with mixed k and with the identity orientation -- prints one JSON line.
  python tools/diffaug_probe.py --blit-ab [--batches 4,32 --repeats 4 --steps 8]
      step time as in --ab, color,translation,cutout vs color,xflip,rot90,translation,cutout.
"""
import argparse
import csv
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

POLICY = "color,translation,cutout"
FULL_POLICY = "color,xflip,rot90,translation,cutout"


def kernels(a):
    from stylegan.pytorch_amd import functional as F
    B, R = a.batch, a.res
    x = torch.randn(B, R, R, 3, device="cuda")
    u = torch.rand(B, 7, device="cuda")
    bits = F.diffaug_policy_bits(POLICY)
    for _ in range(a.iters):
        y = F._diffaug(x, u, bits, False, True)
        F._diffaug(y, u, bits, True, False)
    torch.cuda.synchronize()


def stats(a):
    px = a.batch * a.res * a.res
    bytes_of = {"diffaug_sum_kernel": 12.0 * px, "diffaug_apply_kernel": 24.0 * px}
    rows = []
    with open(a.stats) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            base = next((k for k in bytes_of if k in name), None)
            if base is None:
                continue
            ns = float(r["AverageNs"])
            rows.append(dict(kernel=name, calls=int(r["Calls"]), mean_us=round(ns / 1e3, 2),
                             algorithmic_TBps=round(bytes_of[base] / ns / 1e3, 3)))
    print(json.dumps(dict(batch=a.batch, res=a.res, kernels=rows)))


def ab(a, base="", policy=POLICY):
    import bench
    from stylegan.pytorch_amd import functional as F
    cfg = bench.CONFIGS["ffhq1024"]
    dev = torch.device("cuda:0")
    args = argparse.Namespace(dtype="bf16", graphs="on", alpha=0.5)
    out = dict(box=socket.gethostname(), commit=a.commit, config="ffhq1024", dtype="bf16", graphs=True, policy=policy, base_policy=base,
               blocks=[])
    for B in [int(b) for b in a.batches.split(",")]:
        sg = bench.make_stylegan(args, cfg, dev, None)
        res, depth = cfg["resolution"], cfg["depth"]
        g = torch.Generator(device=dev); g.manual_seed(1234)
        reals = [torch.randn(B, res, res, 3, device=dev, generator=g).permute(0, 3, 1, 2) for _ in range(2)]
        lats = [torch.randn(B, 512, device=dev, generator=g) for _ in range(2)]

        def run(policy, n):
            sg.dis.diffaug_policy, sg.dis._diffaug_bits = policy, F.diffaug_policy_bits(policy)
            torch.cuda.synchronize(); t = time.perf_counter()
            for i in range(n):
                sg.optimize_discriminator(lats[i % 2], reals[i % 2], depth, 0.5)
                sg.optimize_generator(lats[i % 2], reals[i % 2], depth, 0.5)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / n * 1e3

        for p in (base, policy):
            run(p, 4)                                                # 2 eager calls + capture + a replay per half-iteration and policy
        times = {"off": [], "on": []}
        for r in range(a.repeats):
            order = [("off", base), ("on", policy)] if r % 2 == 0 else [("on", policy), ("off", base)]
            for key, p in order:
                times[key].append(run(p, a.steps))
        off, on = min(times["off"]), min(times["on"])
        out["blocks"].append(dict(batch=B, ms_per_step_off=[round(t, 3) for t in times["off"]], ms_per_step_on=[round(t, 3) for t in times["on"]],
                                  best_off=round(off, 3), best_on=round(on, 3), slowdown_pct=round(100 * (on / off - 1), 2)))
        del sg
        torch.cuda.empty_cache()
    print(json.dumps(out))


def _timed(fn, iters, rounds=5):
    """Best-of-``rounds`` mean time in microseconds of ``iters`` back-to-back calls (HIP events on the current stream)."""
    fn(); torch.cuda.synchronize()
    best = float("inf")
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / iters)
    return round(best, 2)


def ada_kernels(a):
    from stylegan.pytorch_amd import functional as F
    R = a.res
    out = dict(box=socket.gethostname(), commit=a.commit, res=R, policy=POLICY, iters=a.iters,
               what="us per call (sum pass + apply kernel, HIP events around back-to-back launches, best of 5)", blocks=[])
    for B in [int(b) for b in a.batches.split(",")]:
        x = torch.randn(B, R, R, 3, device="cuda")
        u = torch.rand(B, 7, device="cuda")
        gates = {"all_on": torch.full((B,), 7, dtype=torch.int32, device="cuda"), "all_off": torch.zeros(B, dtype=torch.int32, device="cuda"),
                 "half_on": (torch.arange(B, device="cuda", dtype=torch.int32) % 2) * 7}
        blk = dict(batch=B)
        for name, adj, bias in (("fwd", False, True), ("adj", True, False)):
            blk[name + "_ungated"] = _timed(lambda: F._diffaug(x, u, 7, adj, bias), a.iters)
            for g, bits in gates.items():
                blk[name + "_gated_" + g] = _timed(lambda: F._diffaug(x, u, 7, adj, bias, bits), a.iters)
            blk[name + "_gated_all_on_vs_ungated_pct"] = round(100 * (blk[name + "_gated_all_on"] / blk[name + "_ungated"] - 1), 2)
        state = torch.tensor([0.5, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device="cuda")
        gu, lg = torch.rand(B, 3, device="cuda"), torch.randn(B, device="cuda")
        blk["ada_gates"] = _timed(lambda: F.ada_gates(gu, state, 7), a.iters)
        blk["ada_update"] = _timed(lambda: F.ada_update(lg, state, 0.6, 1e-12, 4), a.iters)
        out["blocks"].append(blk)
        del x
        torch.cuda.empty_cache()
    print(json.dumps(out))


def blit_kernels(a):
    import statistics
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    R = a.res
    out = dict(box=socket.gethostname(), commit=a.commit, res=R, iters=a.iters,
               what="us per launch of the apply kernel [min, median] (the library's profiler: HIP events around every kernel; the sum "
                    "pass is the same launch shape in every variant and reported once per variant as sum_us)", blocks=[])
    for B in [int(b) for b in a.batches.split(",")]:
        x = torch.randn(B, R, R, 3, device="cuda")
        u = torch.rand(B, 9, device="cuda")
        odd, ident = u.clone(), u.clone()
        odd[:, 8] = torch.where(torch.arange(B, device="cuda") % 2 == 0, 0.3, 0.8)        # k = 1, 3
        ident[:, 7:] = 0
        u7 = u[:, :7].contiguous()
        variants = {"today": (u7, 7), "row_flips": (u, 7 | 8), "tile_k_odd": (odd, 31), "tile_mixed_k": (u, 31), "tile_identity": (ident, 31)}
        blk = dict(batch=B)
        for mode, adj, bias in (("fwd", False, True), ("adj", True, False)):
            for name, (uu, bits) in variants.items():
                F._diffaug(x, uu, bits, adj, bias)                                      # warm
            torch.cuda.synchronize()
            times = {name: dict(apply=[], sum=[]) for name in variants}
            for _ in range(a.iters):
                for name, (uu, bits) in variants.items():
                    N.prof_start(1)
                    F._diffaug(x, uu, bits, adj, bias)
                    torch.cuda.synchronize()
                    N.prof_start(0)
                    for rec in N.prof_records():
                        times[name]["sum" if "_sum" in rec[4].split(" ")[0] else "apply"].append(rec[1] * 1e3)
            for name, t in times.items():
                blk[f"{mode}_{name}"] = [round(min(t["apply"]), 2), round(statistics.median(t["apply"]), 2)]
                blk[f"{mode}_{name}_sum_us"] = round(min(t["sum"]), 2)
            for name in variants:
                if name != "today":
                    blk[f"{mode}_{name}_vs_today"] = round(blk[f"{mode}_{name}"][0] / blk[f"{mode}_today"][0], 3)
        out["blocks"].append(blk)
        del x
        torch.cuda.empty_cache()
    print(json.dumps(out))


def ada_ab(a):
    import bench
    from stylegan.pytorch_amd import functional as F
    cfg = bench.CONFIGS["ffhq1024"]
    dev = torch.device("cuda:0")
    args = argparse.Namespace(dtype="bf16", graphs="on", alpha=0.5)
    out = dict(box=socket.gethostname(), commit=a.commit, config="ffhq1024", dtype="bf16", graphs=True, policy=POLICY,
               what="ms per step, policy alone vs ADA with p pinned to 1", blocks=[])
    for B in [int(b) for b in a.batches.split(",")]:
        sg = bench.make_stylegan(args, cfg, dev, None)
        d = sg.dis
        d.diffaug_policy, d._diffaug_bits = POLICY, F.diffaug_policy_bits(POLICY)
        # ADA's state on the one object: p = 1 and a step of 1e-12 per image (p stays 1); ``d.ada`` switches between the two paths,
        # each with its own captured graphs (the step-graph key holds the ADA configuration)
        d.register_buffer("ada_state", torch.tensor([1.0, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device=dev))
        d.ada_target, d.ada_interval, d.ada_kimg, d._ada_adjust = 0.6, 4, 1e9, 1e-12
        res, depth = cfg["resolution"], cfg["depth"]
        g = torch.Generator(device=dev); g.manual_seed(1234)
        reals = [torch.randn(B, res, res, 3, device=dev, generator=g).permute(0, 3, 1, 2) for _ in range(2)]
        lats = [torch.randn(B, 512, device=dev, generator=g) for _ in range(2)]

        def run(ada, n):
            d.ada = ada
            torch.cuda.synchronize(); t = time.perf_counter()
            for i in range(n):
                sg.optimize_discriminator(lats[i % 2], reals[i % 2], depth, 0.5)
                sg.optimize_generator(lats[i % 2], reals[i % 2], depth, 0.5)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / n * 1e3

        for ada in (False, True):
            run(ada, 4)
        times = {"policy": [], "ada": []}
        for r in range(a.repeats):
            for key in (("policy", "ada") if r % 2 == 0 else ("ada", "policy")):
                times[key].append(run(key == "ada", a.steps))
        off, on = min(times["policy"]), min(times["ada"])
        out["blocks"].append(dict(batch=B, ms_per_step_policy=[round(t, 3) for t in times["policy"]],
                                  ms_per_step_ada=[round(t, 3) for t in times["ada"]], best_policy=round(off, 3), best_ada=round(on, 3),
                                  slowdown_pct=round(100 * (on / off - 1), 2), p_after=float(d.ada_state[0]),
                                  graphs_captured=sum(1 for v in sg._step_graphs.values() if v.graph is not None)))
        del sg
        torch.cuda.empty_cache()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--stats", default=None)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--ada-kernels", action="store_true")
    ap.add_argument("--ada-ab", action="store_true")
    ap.add_argument("--blit-kernels", action="store_true")
    ap.add_argument("--blit-ab", action="store_true")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", default="4,32")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--commit", default=os.environ.get("SGX_COMMIT", ""))
    a = ap.parse_args()
    if a.stats:
        stats(a)
    elif a.kernels:
        kernels(a)
    elif a.ab:
        ab(a)
    elif a.ada_kernels:
        ada_kernels(a)
    elif a.ada_ab:
        ada_ab(a)
    elif a.blit_kernels:
        blit_kernels(a)
    elif a.blit_ab:
        ab(a, base=POLICY, policy=FULL_POLICY)
    else:
        ap.error("one of --kernels, --stats, --ab, --ada-kernels, --ada-ab, --blit-kernels, --blit-ab")


if __name__ == "__main__":
    main()
