"""Image-space corruption probe (csrc/adacorrupt.hip): what ADA's noise + cutout pass costs on the MI355X, and whether the forward
with the in-kernel generator stays at the speed of a read + write stream.

  python tools/corrupt_probe.py [--out profiles/corrupt_probe.json] [--iters 20] [--repeats 4] [--steps 8] [--skip-step]

One process, one JSON document stamped with the box and the commit (--commit or SGX_COMMIT):
  kernels    ``sgx_ada_corrupt`` mode 0 (forward) and mode 1 (linear part) at 1024^2 batch 4 and batch 32, per launch from the library's
             profiler (HIP events around every kernel), [min, median] of ``iters`` calls with the variants interleaved: every image under
             noise + cutout, under noise alone, under the cutout alone, and the identity (the all-zero rows: the copy branch).  The
             yardstick at the same shapes is ``ada_color_vec`` (24 B per pixel in one launch, no generator), interleaved with them.
             Against the bound: 24 B per pixel over 6.3 TB/s.  ``ada_corrupt_table`` is timed alongside ``ada_color_matrix``.
  step       ms per step of ffhq1024, bf16, hipGraph replay (bench.make_stylegan) with the sixteen-op policy against the fourteen-op
             policy, interleaved on ONE StyleGAN object (each policy has its own captured graphs), best of ``repeats``.
  resources  the rows of tools/kernel_resources.py's report for the kernels of adacorrupt.hip (registers, scratch, spills), when the
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

FOURTEEN = "color,xflip,rot90,translation,cutout,scale,rotate,aniso,brightness,contrast,lumaflip,hue,saturation,imgfilter"
SIXTEEN = FOURTEEN + ",noise,imgcutout"
SHAPES = ((1024, 4), (1024, 32))
HBM_BPS = 6.3e12


def kernels(a):
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    blocks = []
    for R, B in SHAPES:
        x = torch.randn(B, R, R, 3, device="cuda")
        u6, gates = torch.rand(B, 6, device="cuda"), torch.rand(B, 2, device="cuda")
        c8, cgates = torch.rand(B, 8, device="cuda"), torch.rand(B, 5, device="cuda")
        state = torch.tensor([0.5, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device="cuda")
        tables = {"noise_cutout": F.ada_corrupt_table(u6, 49152, R, R), "noise": F.ada_corrupt_table(u6, 16384, R, R),
                  "cutout": F.ada_corrupt_table(u6, 32768, R, R), "identity": F.ada_corrupt_table(u6, 0, R, R)}
        cmat = F.ada_color_matrix(c8, 7936)
        px = B * R * R
        blk = dict(res=R, batch=B, MB_moved=round(24.0 * px / 1e6, 2), bound_us=round(24.0 * px / HBM_BPS * 1e6, 2))
        for mode in (0, 1):
            runs = {name: (lambda t=t: F._ada_corrupt(x, t, mode)) for name, t in tables.items()}
            runs["color_vec"] = lambda: F._ada_color(x, cmat, bool(mode), not mode)
            runs["table"] = lambda: F.ada_corrupt_table(u6, 49152, R, R, gates, state)
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
                    recs = [r for r in N.prof_records() if r[4].startswith("ada_")]
                    assert len(recs) == 1, recs
                    times[name].append(recs[0][1] * 1e3)
                    names[name] = recs[0][4]
            blk[f"mode{mode}_launches"] = names
            for name, t in times.items():
                blk[f"mode{mode}_{name}_us"] = [round(min(t), 2), round(statistics.median(t), 2)]
            for name in tables:
                best = blk[f"mode{mode}_{name}_us"][0]
                blk[f"mode{mode}_{name}_vs_color_vec"] = round(best / blk[f"mode{mode}_color_vec_us"][0], 3)
                blk[f"mode{mode}_{name}_share_of_hbm_bound"] = round(blk["bound_us"] / best, 3)
            blk[f"mode{mode}_table_vs_color_matrix"] = round(blk[f"mode{mode}_table_us"][0] / blk[f"mode{mode}_color_matrix_us"][0], 3)
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

        for p in (FOURTEEN, SIXTEEN):
            run(p, 4)                                                # 2 eager calls + capture + a replay per half-iteration and policy
        times = {"fourteen": [], "sixteen": []}
        for r in range(a.repeats):
            order = [("fourteen", FOURTEEN), ("sixteen", SIXTEEN)] if r % 2 == 0 else [("sixteen", SIXTEEN), ("fourteen", FOURTEEN)]
            for key, p in order:
                times[key].append(run(p, a.steps))
        t14, t16 = min(times["fourteen"]), min(times["sixteen"])
        blocks.append(dict(batch=B, ms_per_step_fourteen=[round(t, 3) for t in times["fourteen"]],
                           ms_per_step_sixteen=[round(t, 3) for t in times["sixteen"]], best_fourteen=round(t14, 3),
                           best_sixteen=round(t16, 3), slowdown_pct=round(100 * (t16 / t14 - 1), 2),
                           graphs_captured=sum(1 for v in sg._step_graphs.values() if v.graph is not None)))
        del sg
        torch.cuda.empty_cache()
    return blocks


def resources():
    import kernel_resources
    keys = ("name", "vgpr", "sgpr", "scratch", "occupancy", "sgpr_spill", "vgpr_spill", "static_lds")
    return [{k: r.get(k) for k in keys} for r in kernel_resources.collect() if r["file"] == "adacorrupt.hip"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corrupt_probe.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="4,32")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--commit", default=os.environ.get("SGX_COMMIT", ""))
    a = ap.parse_args()
    out = dict(box=socket.gethostname(), commit=a.commit, device=torch.cuda.get_device_name(0), iters=a.iters,
               what="kernels: us per launch [min, median] from the library's profiler, variants interleaved; bound_us: 24 B per pixel over "
                    "6.3 TB/s; step: ms per step of ffhq1024 bf16 under hipGraph replay, every image under the whole policy (no ADA gates), "
                    "best of `repeats`; resources: the compiler's remarks for adacorrupt.hip",
               kernels=kernels(a), resources=resources())
    if not a.skip_step:
        out["step"] = dict(config="ffhq1024", dtype="bf16", graphs=True, fourteen=FOURTEEN, sixteen=SIXTEEN, repeats=a.repeats, steps=a.steps,
                           blocks=step(a))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
