"""Geometric-stage probe (csrc/adageom.hip): what ADA's scale / rotate / aniso resample costs on the MI355X.

  python tools/geom_probe.py [--out profiles/geom_probe.json] [--iters 20] [--repeats 4] [--steps 8] [--skip-step]
  python tools/geom_probe.py --padding reflect [--out profiles/geom_pad_probe.json] ...      (csrc/adageompad.hip against adageom.hip)

One process, one JSON document stamped with the box and the commit (--commit or SGX_COMMIT):
  kernels   ``sgx_ada_geom`` forward and adjoint at 1024^2 batch 4 and batch 32 and at 128^2 batch 64, per launch from the library's
            profiler (HIP events around every kernel), [min, median] of ``iters`` launches with the variants interleaved: every row of
            the table the identity (the copy branch), the rows of a random draw gated at p = 0.5, and every row at the widest adjoint
            window the clamp allows (T = Rot diag(2^1.2, 1) at the angle that maximises |t00| + |t01|).  The yardstick is the
            ``diffaug_blit_tile`` apply launch on the same tensors in the same rounds; ``ada_geom_matrix`` is timed alongside.
  step      ms per step of ffhq1024, bf16, hipGraph replay (bench.make_stylegan) with the eight-op policy against the five-op policy,
            interleaved on ONE StyleGAN object (each policy has its own captured graphs), best of ``repeats``.
With ``--padding reflect`` the document compares the two padding modes instead:
  kernels   ``sgx_ada_geom_reflect`` against ``sgx_ada_geom`` at 1024^2 batch 4 and 32, forward and adjoint, under the mixed table and
            under the widest-window row, interleaved, [min, median] of ``iters`` launches and the ratio of the minima; the compiler's
            resource remarks for adageompad.hip when the tree was built by make.
  step      ms per step of ffhq1024, bf16, hipGraph replay under the eight-op policy, geom_padding "reflect" against "zeros": one
            StyleGAN object per mode (the mode is fixed for a model's lifetime), interleaved, best of ``repeats``."""
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


def pad_kernels(a):
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    blocks = []
    for R, B in SHAPES[:2]:
        x = torch.randn(B, R, R, 3, device="cuda")
        u5, gates = torch.rand(B, 5, device="cuda"), torch.rand(B, 3, device="cuda")
        state = torch.tensor([0.5, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device="cuda")
        tables = {"mixed_p0.5": F.ada_geom_matrix(u5, 224, gates, state), "widest_window": torch.from_numpy(np.stack([widest_row()] * B)).cuda()}
        ident = sum(1 for r in tables["mixed_p0.5"].cpu().tolist() if r == [1, 0, 0, 1, 1, 0, 0, 1])
        blk = dict(res=R, batch=B, mixed_identity_rows=ident, MB_moved=round(24.0 * B * R * R / 1e6, 2))
        for mode, adj in (("fwd", False), ("adj", True)):
            runs = {f"{name}_{pad}": (lambda m=m, e=e: F._ada_geom(x, m, adj, e)) for name, m in tables.items()
                    for pad, e in (("zeros", "sgx_ada_geom"), ("reflect", "sgx_ada_geom_reflect"))}
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
                    recs = N.prof_records()
                    assert len(recs) == 1 and recs[0][4].startswith("ada_geom_reflect_tile" if name.endswith("reflect") else "ada_geom_tile"), recs
                    times[name].append(recs[0][1] * 1e3)
            for name, t in times.items():
                blk[f"{mode}_{name}_us"] = [round(min(t), 2), round(statistics.median(t), 2)]
            for name in tables:
                blk[f"{mode}_{name}_reflect_vs_zeros"] = round(blk[f"{mode}_{name}_reflect_us"][0] / blk[f"{mode}_{name}_zeros_us"][0], 3)
        blocks.append(blk)
        del x
        torch.cuda.empty_cache()
    return blocks


def pad_step(a):
    import bench
    cfg = bench.CONFIGS["ffhq1024"]
    dev = torch.device("cuda:0")
    args = argparse.Namespace(dtype="bf16", graphs="on", alpha=0.5)
    blocks = []
    for B in [int(b) for b in a.batches.split(",")]:
        res, depth = cfg["resolution"], cfg["depth"]
        g = torch.Generator(device=dev); g.manual_seed(1234)
        reals = [torch.randn(B, res, res, 3, device=dev, generator=g).permute(0, 3, 1, 2) for _ in range(2)]
        lats = [torch.randn(B, 512, device=dev, generator=g) for _ in range(2)]
        sgs = {}
        for pad in ("zeros", "reflect"):                             # the mode is fixed at construction: one model (and its graphs) per mode
            sg = bench.make_stylegan(args, cfg, dev, None)
            from stylegan.pytorch_amd import functional as F
            sg.dis.diffaug_policy, sg.dis._diffaug_bits, sg.dis.geom_padding = EIGHT, F.diffaug_policy_bits(EIGHT), pad
            sgs[pad] = sg

        def run(pad, n):
            sg = sgs[pad]
            torch.cuda.synchronize(); t = time.perf_counter()
            for i in range(n):
                sg.optimize_discriminator(lats[i % 2], reals[i % 2], depth, 0.5)
                sg.optimize_generator(lats[i % 2], reals[i % 2], depth, 0.5)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / n * 1e3

        for pad in sgs:
            run(pad, 4)                                              # 2 eager calls + capture + a replay per half-iteration
        times = {pad: [] for pad in sgs}
        for r in range(a.repeats):
            for pad in (("zeros", "reflect") if r % 2 == 0 else ("reflect", "zeros")):
                times[pad].append(run(pad, a.steps))
        zeros, reflect = min(times["zeros"]), min(times["reflect"])
        blocks.append(dict(batch=B, ms_per_step_zeros=[round(t, 3) for t in times["zeros"]], ms_per_step_reflect=[round(t, 3) for t in times["reflect"]],
                           best_zeros=round(zeros, 3), best_reflect=round(reflect, 3), slowdown_pct=round(100 * (reflect / zeros - 1), 2),
                           graphs_captured={pad: sum(1 for v in sg._step_graphs.values() if v.graph is not None) for pad, sg in sgs.items()}))
        del sgs
        torch.cuda.empty_cache()
    return blocks


def pad_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    keys = ("name", "vgpr", "agpr", "sgpr", "scratch", "vgpr_spill", "sgpr_spill", "occupancy", "static_lds")
    return [{k: r.get(k) for k in keys} for r in kernel_resources.collect() if r["file"] == "adageompad.hip"]


def pad_main(a):
    out = dict(box=socket.gethostname(), commit=a.commit, device=torch.cuda.get_device_name(0), iters=a.iters,
               what="kernels: us per launch [min, median] from the library's profiler, sgx_ada_geom_reflect and sgx_ada_geom interleaved on "
                    "the same tensors and tables, *_reflect_vs_zeros the ratio of the minima; step: ms per step of ffhq1024 bf16 under "
                    "hipGraph replay, eight-op policy, every image under every op, best of `repeats`; resources: the compiler's remarks "
                    "for adageompad.hip",
               kernels=pad_kernels(a), resources=pad_resources())
    if a.skip_step:
        out["step"] = dict(not_measured=True, command="python tools/geom_probe.py --padding reflect --batches 4,32 --repeats 4")
    else:
        out["step"] = dict(config="ffhq1024", dtype="bf16", graphs=True, policy=EIGHT, repeats=a.repeats, steps=a.steps, blocks=pad_step(a))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--padding", choices=("zeros", "reflect"), default="zeros")
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="4,32")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--commit", default=os.environ.get("SGX_COMMIT", ""))
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "geom_pad_probe.json" if a.padding == "reflect" else "geom_probe.json")
    if a.padding == "reflect":
        return write(a, pad_main(a))
    out = dict(box=socket.gethostname(), commit=a.commit, device=torch.cuda.get_device_name(0), iters=a.iters,
               what="kernels: us per launch [min, median] from the library's profiler, variants interleaved; step: ms per step of ffhq1024 "
                    "bf16 under hipGraph replay, every image under the whole policy (no ADA gates), best of `repeats`",
               kernels=kernels(a))
    if not a.skip_step:
        out["step"] = dict(config="ffhq1024", dtype="bf16", graphs=True, five=FIVE, eight=EIGHT, repeats=a.repeats, steps=a.steps, blocks=step(a))
    write(a, out)


def write(a, out):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
