"""Image-space filtering probe (csrc/adafilter.hip): what ADA's imgfilter pass costs on the MI355X, and which bound applies to it.

  python tools/filter_probe.py [--out profiles/filter_probe.json] [--iters 20] [--repeats 4] [--steps 8] [--skip-step]

One process, one JSON document stamped with the box and the commit (--commit or SGX_COMMIT):
  kernels    ``sgx_ada_filter`` forward and adjoint at 1024^2 batch 4 and batch 32 and at 128^2 batch 64, per launch from the library's
             profiler (HIP events around every kernel), [min, median] of ``iters`` calls with the variants interleaved: every row of the
             table the identity (the copy branch), the rows of a random draw gated at p = 0.5, and every row drawn.  A call is two
             launches (one axis each); both are listed, and their sum.  The yardsticks at the same shapes are ``ada_geom_tile`` and
             ``ada_color_vec``, which move 24 B per pixel in one launch, each right behind a read of its input.  Against the two
             bounds: bytes (24 B per pixel and launch) over 6.3 TB/s, and 516 fp32 operations per pixel and call (2 axes x 43 taps x
             multiply and add x 3 channels) over the 157.3 TFLOP/s vector peak; the form the kernels use (the symmetric pairing:
             1 multiply, 21 adds, 21 fused multiply-adds per output and axis = 258 vector instructions per pixel) against the
             78.6 T lane-instructions/s the unpacked fp32 pipe issues.  ``ada_filter_matrix`` is timed alongside ``ada_color_matrix``.
  step       ms per step of ffhq1024, bf16, hipGraph replay (bench.make_stylegan) with the fourteen-op policy against the thirteen-op
             policy, interleaved on ONE StyleGAN object (each policy has its own captured graphs), best of ``repeats``.
  resources  the rows of tools/kernel_resources.py's report for the kernels of adafilter.hip (registers, scratch, spills), when the
             build's resource remarks are there."""
import argparse
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

THIRTEEN = "color,xflip,rot90,translation,cutout,scale,rotate,aniso,brightness,contrast,lumaflip,hue,saturation"
FOURTEEN = THIRTEEN + ",imgfilter"
SHAPES = ((1024, 4), (1024, 32), (128, 64))
HBM_BPS, FP32_FLOPS, FP32_ISSUE = 6.3e12, 157.3e12, 78.65e12


def kernels(a):
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    blocks = []
    for R, B in SHAPES:
        x = torch.randn(B, R, R, 3, device="cuda")
        u8, gates = torch.rand(B, 8, device="cuda"), torch.rand(B, 4, device="cuda")
        c8, cgates = torch.rand(B, 8, device="cuda"), torch.rand(B, 5, device="cuda")
        u5 = torch.rand(B, 5, device="cuda")
        state = torch.tensor([0.5, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device="cuda")
        tables = {"identity": F.ada_filter_matrix(u8, 0), "mixed_p0.5": F.ada_filter_matrix(u8, 8192, gates, state),
                  "drawn": F.ada_filter_matrix(u8, 8192)}
        ident = sum(1 for r in tables["mixed_p0.5"].cpu().tolist() if r == [1.0] + [0.0] * 21)
        gmat, cmat = F.ada_geom_matrix(u5, 224), F.ada_color_matrix(c8, 7936)
        px = B * R * R
        blk = dict(res=R, batch=B, mixed_identity_rows=ident, MB_moved_per_launch=round(24.0 * px / 1e6, 2),
                   bound_us=dict(hbm_per_launch=round(24.0 * px / HBM_BPS * 1e6, 2), hbm_per_call=round(48.0 * px / HBM_BPS * 1e6, 2),
                                 fp32_516_ops_per_call=round(516.0 * px / FP32_FLOPS * 1e6, 2),
                                 issue_258_instr_per_call=round(258.0 * px / FP32_ISSUE * 1e6, 2)))
        for mode, adj in (("fwd", False), ("adj", True)):
            runs = {name: (lambda m=m: F._ada_filter(x, m, adj)) for name, m in tables.items()}
            # the yardsticks right behind a read of their input (profiles/color_probe.json: where a stage's pass stands in the step)
            runs["geom_tile"] = lambda: (x.sum(), F._ada_geom(x, gmat, adj))
            runs["color_vec"] = lambda: (x.sum(), F._ada_color(x, cmat, adj, not adj))
            runs["drawn_after_read"] = lambda: (x.sum(), F._ada_filter(x, tables["drawn"], adj))
            runs["matrix"] = lambda: F.ada_filter_matrix(u8, 8192, gates, state)
            runs["color_matrix"] = lambda: F.ada_color_matrix(c8, 7936, cgates, state)
            for fn in runs.values():
                fn()                                                                    # warm
            torch.cuda.synchronize()
            times, names = {name: [] for name in runs}, {}
            for _ in range(a.iters):
                for name, fn in runs.items():
                    N.prof_start(1)
                    fn()
                    torch.cuda.synchronize()
                    N.prof_start(0)
                    recs = [r for r in N.prof_records() if r[4].startswith(("ada_", "diffaug"))]
                    assert len(recs) == (2 if "ada_filter_" in recs[0][4] and "matrix" not in recs[0][4] else 1), recs
                    times[name].append([r[1] * 1e3 for r in recs])
                    names[name] = [r[4] for r in recs]
            blk[f"{mode}_launches"] = names
            for name, t in times.items():
                tot = [sum(v) for v in t]
                blk[f"{mode}_{name}_us"] = [round(min(tot), 2), round(statistics.median(tot), 2)]
                if len(t[0]) == 2:
                    blk[f"{mode}_{name}_us_per_launch"] = [round(min(v[k] for v in t), 2) for k in range(2)]
            for name in list(tables) + ["drawn_after_read"]:
                for yard in ("geom_tile", "color_vec"):
                    blk[f"{mode}_{name}_vs_{yard}"] = round(blk[f"{mode}_{name}_us"][0] / blk[f"{mode}_{yard}_us"][0], 3)
            best = blk[f"{mode}_drawn_us"][0]
            b = blk["bound_us"]
            blk[f"{mode}_drawn_share_of_peak"] = dict(
                least_us=max(b["hbm_per_call"], b["fp32_516_ops_per_call"]), bound="hbm" if b["hbm_per_call"] >= b["fp32_516_ops_per_call"] else "fp32",
                share=round(max(b["hbm_per_call"], b["fp32_516_ops_per_call"]) / best, 3), issue_share=round(b["issue_258_instr_per_call"] / best, 3))
            blk[f"{mode}_matrix_vs_color_matrix"] = round(blk[f"{mode}_matrix_us"][0] / blk[f"{mode}_color_matrix_us"][0], 3)
        blocks.append(blk)
        del x
        torch.cuda.empty_cache()
    return blocks


def step(a):
    import bench
    from stylegan.pytorch_amd import functional as F
    cfg = bench.CONFIGS["ffhq1024"]
    dev = torch.device("cuda:0")
    args = argparse.Namespace(dtype="bf16", graphs="on", alpha=0.5)
    blocks = []
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

        for p in (THIRTEEN, FOURTEEN):
            run(p, 4)                                                # 2 eager calls + capture + a replay per half-iteration and policy
        times = {"thirteen": [], "fourteen": []}
        for r in range(a.repeats):
            order = [("thirteen", THIRTEEN), ("fourteen", FOURTEEN)] if r % 2 == 0 else [("fourteen", FOURTEEN), ("thirteen", THIRTEEN)]
            for key, p in order:
                times[key].append(run(p, a.steps))
        t13, t14 = min(times["thirteen"]), min(times["fourteen"])
        blocks.append(dict(batch=B, ms_per_step_thirteen=[round(t, 3) for t in times["thirteen"]],
                           ms_per_step_fourteen=[round(t, 3) for t in times["fourteen"]], best_thirteen=round(t13, 3),
                           best_fourteen=round(t14, 3), slowdown_pct=round(100 * (t14 / t13 - 1), 2),
                           graphs_captured=sum(1 for v in sg._step_graphs.values() if v.graph is not None)))
        del sg
        torch.cuda.empty_cache()
    return blocks


def resources():
    import kernel_resources
    keys = ("name", "vgpr", "sgpr", "scratch", "occupancy", "sgpr_spill", "vgpr_spill", "static_lds")
    return [{k: r.get(k) for k in keys} for r in kernel_resources.collect() if r["file"] == "adafilter.hip"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_probe.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="4,32")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--commit", default=os.environ.get("SGX_COMMIT", ""))
    a = ap.parse_args()
    out = dict(box=socket.gethostname(), commit=a.commit, device=torch.cuda.get_device_name(0), iters=a.iters,
               what="kernels: us per call (two launches) [min, median] from the library's profiler, variants interleaved, the yardsticks "
                    "behind a read of their input; bound_us: the least time by each bound; step: ms per step of ffhq1024 bf16 under hipGraph "
                    "replay, every image under the whole policy (no ADA gates), best of `repeats`; resources: the compiler's remarks for "
                    "adafilter.hip",
               kernels=kernels(a), resources=resources())
    if not a.skip_step:
        out["step"] = dict(config="ffhq1024", dtype="bf16", graphs=True, thirteen=THIRTEEN, fourteen=FOURTEEN, repeats=a.repeats, steps=a.steps,
                           blocks=step(a))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
