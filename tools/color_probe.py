"""Colour-stage probe (csrc/adacolor.hip): what ADA's brightness / contrast / lumaflip / hue / saturation pass costs on the MI355X.

  python tools/color_probe.py [--out profiles/color_probe.json] [--iters 20] [--repeats 4] [--steps 8] [--skip-step]

One process, one JSON document stamped with the box and the commit (--commit or SGX_COMMIT):
  kernels    ``sgx_ada_color`` forward and adjoint at 1024^2 batch 4 and batch 32 and at 128^2 batch 64, per launch from the library's
             profiler (HIP events around every kernel), [min, median] of ``iters`` launches with the variants interleaved: every row of
             the table the identity (the copy branch), the rows of a random draw gated at p = 0.5, and every row drawn (no gates; also right
             behind a read of the input, ``drawn_after_read``, which is where the yardsticks' apply launch stands: behind its sum pass).  The
             yardstick is the apply launch of section 9 on the same tensors in the same rounds: ``diffaug_blit_row`` under
             ``color,xflip`` and the plain ``diffaug`` apply kernel under ``color``, which move 24 B per pixel like the colour pass;
             the same two under ``color,xflip,translation,cutout`` / ``color,translation,cutout`` are listed as well (``*_masked``:
             they do not load the pixels the cutout and the padding zero, a quarter of the reads and more).  ``ada_color_matrix``
             is timed alongside ``ada_geom_matrix``.
  step       ms per step of ffhq1024, bf16, hipGraph replay (bench.make_stylegan) with the thirteen-op policy against the eight-op
             policy, interleaved on ONE StyleGAN object (each policy has its own captured graphs), best of ``repeats``.
  resources  the rows of tools/kernel_resources.py's report for the kernels of adacolor.hip (registers, scratch, spills), when the
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

EIGHT = "color,xflip,rot90,translation,cutout,scale,rotate,aniso"
THIRTEEN = EIGHT + ",brightness,contrast,lumaflip,hue,saturation"
SHAPES = ((1024, 4), (1024, 32), (128, 64))
COLOR_MASK = 7936


def kernels(a):
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    blocks = []
    for R, B in SHAPES:
        x = torch.randn(B, R, R, 3, device="cuda")
        u9, u7 = torch.rand(B, 9, device="cuda"), torch.rand(B, 7, device="cuda")
        u8, gates = torch.rand(B, 8, device="cuda"), torch.rand(B, 5, device="cuda")
        u5, gates3 = torch.rand(B, 5, device="cuda"), torch.rand(B, 3, device="cuda")
        state = torch.tensor([0.5, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device="cuda")
        tables = {"identity": F.ada_color_matrix(u8, 0), "mixed_p0.5": F.ada_color_matrix(u8, COLOR_MASK, gates, state),
                  "drawn": F.ada_color_matrix(u8, COLOR_MASK)}
        ident = sum(1 for r in tables["mixed_p0.5"].cpu().tolist() if r == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
        blk = dict(res=R, batch=B, mixed_identity_rows=ident, MB_moved=round(24.0 * B * R * R / 1e6, 2))
        for mode, adj in (("fwd", False), ("adj", True)):
            runs = {name: (lambda m=m: F._ada_color(x, m, adj, not adj)) for name, m in tables.items()}
            # the yardsticks' apply launch runs behind their own sum pass, which has just read x: the same pass behind a read of x
            runs["drawn_after_read"] = lambda: (x.sum(), F._ada_color(x, tables["drawn"], adj, not adj))
            runs["blit_row"] = lambda: F._diffaug(x, u9, 1 | 8, adj, not adj)              # color,xflip
            runs["apply"] = lambda: F._diffaug(x, u7, 1, adj, not adj)                     # color
            runs["blit_row_masked"] = lambda: F._diffaug(x, u9, 1 | 8 | 2 | 4, adj, not adj)   # color,xflip,translation,cutout
            runs["apply_masked"] = lambda: F._diffaug(x, u7, 7, adj, not adj)              # color,translation,cutout
            runs["matrix"] = lambda: F.ada_color_matrix(u8, COLOR_MASK, gates, state)
            runs["geom_matrix"] = lambda: F.ada_geom_matrix(u5, 224, gates3, state)
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
                    recs = [r for r in N.prof_records() if "_sum" not in r[4].split(" ")[0]]   # (the apply launch's sum pass is not the yardstick)
                    assert len(recs) == 1, recs
                    times[name].append(recs[0][1] * 1e3)
                    names[name] = recs[0][4].split(" ")[0]
            blk[f"{mode}_launches"] = names
            for name, t in times.items():
                blk[f"{mode}_{name}_us"] = [round(min(t), 2), round(statistics.median(t), 2)]
            for name in list(tables) + ["drawn_after_read"]:
                for yard in ("blit_row", "apply", "blit_row_masked", "apply_masked"):
                    blk[f"{mode}_{name}_vs_{yard}"] = round(blk[f"{mode}_{name}_us"][0] / blk[f"{mode}_{yard}_us"][0], 3)
            blk[f"{mode}_matrix_vs_geom_matrix"] = round(blk[f"{mode}_matrix_us"][0] / blk[f"{mode}_geom_matrix_us"][0], 3)
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

        for p in (EIGHT, THIRTEEN):
            run(p, 4)                                                # 2 eager calls + capture + a replay per half-iteration and policy
        times = {"eight": [], "thirteen": []}
        for r in range(a.repeats):
            order = [("eight", EIGHT), ("thirteen", THIRTEEN)] if r % 2 == 0 else [("thirteen", THIRTEEN), ("eight", EIGHT)]
            for key, p in order:
                times[key].append(run(p, a.steps))
        eight, thirteen = min(times["eight"]), min(times["thirteen"])
        blocks.append(dict(batch=B, ms_per_step_eight=[round(t, 3) for t in times["eight"]],
                           ms_per_step_thirteen=[round(t, 3) for t in times["thirteen"]], best_eight=round(eight, 3),
                           best_thirteen=round(thirteen, 3), slowdown_pct=round(100 * (thirteen / eight - 1), 2),
                           graphs_captured=sum(1 for v in sg._step_graphs.values() if v.graph is not None)))
        del sg
        torch.cuda.empty_cache()
    return blocks


def resources():
    import kernel_resources
    keys = ("name", "vgpr", "sgpr", "scratch", "occupancy", "sgpr_spill", "vgpr_spill", "static_lds")
    return [{k: r.get(k) for k in keys} for r in kernel_resources.collect() if r["file"] == "adacolor.hip"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_probe.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="4,32")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--commit", default=os.environ.get("SGX_COMMIT", ""))
    a = ap.parse_args()
    out = dict(box=socket.gethostname(), commit=a.commit, device=torch.cuda.get_device_name(0), iters=a.iters,
               what="kernels: us per launch [min, median] from the library's profiler, variants interleaved; step: ms per step of ffhq1024 "
                    "bf16 under hipGraph replay, every image under the whole policy (no ADA gates), best of `repeats`; resources: the "
                    "compiler's remarks for adacolor.hip",
               kernels=kernels(a), resources=resources())
    if not a.skip_step:
        out["step"] = dict(config="ffhq1024", dtype="bf16", graphs=True, eight=EIGHT, thirteen=THIRTEEN, repeats=a.repeats, steps=a.steps,
                           blocks=step(a))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
