"""Geometric-stage probe (csrc/adageom.hip): what ADA's scale / rotate / aniso resample costs on the MI355X.

  python tools/geom_probe.py [--out profiles/geom_probe.json] [--iters 20] [--repeats 4] [--steps 8] [--skip-step]

One process, one JSON document stamped with the box and the commit (--commit or SGX_COMMIT):
  kernels   ``sgx_ada_geom`` forward and adjoint at 1024^2 batch 4 and batch 32 and at 128^2 batch 64, per launch from the library's
            profiler (HIP events around every kernel), [min, median] of ``iters`` launches with the variants interleaved: every row of
            the table the identity (the copy branch), the rows of a random draw gated at p = 0.5, and every row at the widest adjoint
            window the clamp allows (T = Rot diag(2^1.2, 1) at the angle that maximises |t00| + |t01|).  The yardstick is the
            ``diffaug_blit_tile`` apply launch on the same tensors in the same rounds; ``ada_geom_matrix`` is timed alongside.
  step      ms per step of ffhq1024, bf16, hipGraph replay (bench.make_stylegan) with the eight-op policy against the five-op policy,
            interleaved on ONE StyleGAN object (each policy has its own captured graphs), best of ``repeats``."""
import argparse
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FIVE = "color,xflip,rot90,translation,cutout"
EIGHT = FIVE + ",scale,rotate,aniso"
SHAPES = ((1024, 4), (1024, 32), (128, 64))


def widest_row():
    big = 2.0 ** 1.2
    t = np.arctan(1.0 / big)
    T = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]) @ np.diag([big, 1.0])
    return np.concatenate([np.linalg.inv(T).reshape(-1), T.reshape(-1)]).astype(np.float32)


def kernels(a):
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    blocks = []
    for R, B in SHAPES:
        x = torch.randn(B, R, R, 3, device="cuda")
        u9 = torch.rand(B, 9, device="cuda")
        u5, gates = torch.rand(B, 5, device="cuda"), torch.rand(B, 3, device="cuda")
        state = torch.tensor([0.5, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device="cuda")
        tables = {"identity": F.ada_geom_matrix(u5, 0), "mixed_p0.5": F.ada_geom_matrix(u5, 224, gates, state),
                  "widest_window": torch.from_numpy(np.stack([widest_row()] * B)).cuda()}
        ident = sum(1 for r in tables["mixed_p0.5"].cpu().tolist() if r == [1, 0, 0, 1, 1, 0, 0, 1])
        blk = dict(res=R, batch=B, mixed_identity_rows=ident, MB_moved=round(24.0 * B * R * R / 1e6, 2))
        for mode, adj in (("fwd", False), ("adj", True)):
            runs = {name: (lambda m=m: F._ada_geom(x, m, adj)) for name, m in tables.items()}
            runs["blit_tile"] = lambda: F._diffaug(x, u9, 31, adj, not adj)
            runs["matrix"] = lambda: F.ada_geom_matrix(u5, 224, gates, state)
            for fn in runs.values():
                fn()                                                                    # warm
            torch.cuda.synchronize()
            times = {name: [] for name in runs}
            for _ in range(a.iters):
                for name, fn in runs.items():
                    N.prof_start(1)
                    fn()
                    torch.cuda.synchronize()
                    N.prof_start(0)
                    recs = [r for r in N.prof_records() if "_sum" not in r[4].split(" ")[0]]   # (the blit launch's sum pass is not the yardstick)
                    assert len(recs) == 1, recs
                    times[name].append(recs[0][1] * 1e3)
            for name, t in times.items():
                blk[f"{mode}_{name}_us"] = [round(min(t), 2), round(statistics.median(t), 2)]
            for name in tables:
                blk[f"{mode}_{name}_vs_blit_tile"] = round(blk[f"{mode}_{name}_us"][0] / blk[f"{mode}_blit_tile_us"][0], 3)
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

        for p in (FIVE, EIGHT):
            run(p, 4)                                                # 2 eager calls + capture + a replay per half-iteration and policy
        times = {"five": [], "eight": []}
        for r in range(a.repeats):
            order = [("five", FIVE), ("eight", EIGHT)] if r % 2 == 0 else [("eight", EIGHT), ("five", FIVE)]
            for key, p in order:
                times[key].append(run(p, a.steps))
        five, eight = min(times["five"]), min(times["eight"])
        blocks.append(dict(batch=B, ms_per_step_five=[round(t, 3) for t in times["five"]], ms_per_step_eight=[round(t, 3) for t in times["eight"]],
                           best_five=round(five, 3), best_eight=round(eight, 3), slowdown_pct=round(100 * (eight / five - 1), 2),
                           graphs_captured=sum(1 for v in sg._step_graphs.values() if v.graph is not None)))
        del sg
        torch.cuda.empty_cache()
    return blocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geom_probe.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="4,32")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--commit", default=os.environ.get("SGX_COMMIT", ""))
    a = ap.parse_args()
    out = dict(box=socket.gethostname(), commit=a.commit, device=torch.cuda.get_device_name(0), iters=a.iters,
               what="kernels: us per launch [min, median] from the library's profiler, variants interleaved; step: ms per step of ffhq1024 "
                    "bf16 under hipGraph replay, every image under the whole policy (no ADA gates), best of `repeats`",
               kernels=kernels(a))
    if not a.skip_step:
        out["step"] = dict(config="ffhq1024", dtype="bf16", graphs=True, five=FIVE, eight=EIGHT, repeats=a.repeats, steps=a.steps, blocks=step(a))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
