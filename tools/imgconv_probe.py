#!/usr/bin/env python3
"""Times the image-side 1x1 kernels of csrc/imgconv.hip (J = 1 and 4 image channels) next to the 3-channel kernels of csrc/pointwise.hip
at the two image-end shapes of the headline step (B = 4: 1024^2 x 16 and 512^2 x 32, bf16), and judges them:

  J = 1: at most 1.10 x its 3-channel counterpart;  J = 4: at most 1.10 x bytes(J=4) / bytes(J=3) x it (bytes as SGX_NOTE counts them:
  npix (4 J + 2 C)).  10 % = the ~5 % same-code spread between boxes, doubled for us-scale launches.

Method: every kernel warmed up, then ``--iters`` rounds; a round launches each kernel once, in turn (interleaved), each launch between two
events on the one stream; the figure is the median over the rounds.

  python tools/imgconv_probe.py [--iters 30] [--commit SHA] [--out profiles/imgconv_probe.json]
  python tools/imgconv_probe.py --sweep        loop kernel against short-lived blocks around the launchers' size threshold: runs itself
                                               once with SGX_IMG1_MIN=0 (the switch is read once per process) and prints both columns"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from stylegan.pytorch_amd import native as N  # noqa: E402

DEV = "cuda:0"


def kernels(L, npix, C, dt):
    """name -> (launch closure, J, kind)."""
    st = N.stream
    x = torch.randn(npix, C, device=DEV).to(dt)
    y = torch.empty(npix, C, device=DEV, dtype=dt)
    dtc = N.dt(x)
    out = {}
    for J in (3, 1, 4):
        img = torch.randn(npix, J, device=DEV)
        io = torch.empty(npix, J, device=DEV)
        w = torch.randn(C, J, 1, 1, device=DEV)
        b, bj = torch.randn(C, device=DEV), torch.randn(J, device=DEV)
        dw = torch.empty_like(w)
        p = lambda t: t.data_ptr()
        if J == 3:
            ws = N.workspace(L.sgx_rgb_wgrad_ws_bytes(npix, C), DEV)
            out["in", J] = lambda img=img, w=w, b=b: L.sgx_rgb_in(p(img), p(w), 1, 3, 0.5, p(b), p(y), npix, C, dtc, st())
            out["out", J] = lambda io=io, w=w, bj=bj: L.sgx_rgb_out(p(x), p(w), 1, 3, 0.5, p(bj), p(io), npix, C, dtc, st())
            out["wgrad", J] = lambda img=img, dw=dw, ws=ws: L.sgx_rgb_wgrad(p(img), p(x), p(dw), 1, 3, 0.5, p(ws), ws.numel(), npix, C, dtc, st())
        else:
            ws = N.workspace(L.sgx_img_wgrad_ws_bytes(npix, J, C), DEV)
            out["in", J] = lambda img=img, w=w, b=b, J=J: L.sgx_img_in(p(img), p(w), J, 1, J, 0.5, p(b), p(y), npix, C, dtc, st())
            out["out", J] = lambda io=io, w=w, bj=bj, J=J: L.sgx_img_out(p(x), p(w), J, 1, J, 0.5, p(bj), p(io), npix, C, dtc, st())
            out["wgrad", J] = lambda img=img, dw=dw, ws=ws, J=J: L.sgx_img_wgrad(p(img), p(x), p(dw), J, 1, J, 0.5, p(ws), ws.numel(), npix, C, dtc, st())
    return out


def medians(ks, iters):
    for fn in ks.values():
        for _ in range(5):
            N.check(fn(), "warm-up")
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in ks}
    for i in range(iters):
        for k, fn in ks.items():                                            # interleaved: one launch of each kernel per round
            ev[k][i][0].record()
            N.check(fn(), "launch")
            ev[k][i][1].record()
    torch.cuda.synchronize()
    return {k: statistics.median(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in ev.items()}


def judge(a):
    L = N.lib()
    rows, ok = [], True
    for B, R, C in ((4, 1024, 16), (4, 512, 32)):
        npix = B * R * R
        us = medians(kernels(L, npix, C, torch.bfloat16), a.iters)
        for kind in ("in", "out", "wgrad"):
            for J in (1, 4):
                ratio = 1.0 if J == 1 else (4.0 * J + 2.0 * C) / (12.0 + 2.0 * C)
                limit = 1.10 * ratio * us[kind, 3]
                row = dict(shape=f"B{B} {R}x{R} C{C} bf16", kernel=f"img_{kind}", J=J, us=round(us[kind, J], 2), rgb_us=round(us[kind, 3], 2),
                           bytes_ratio=round(ratio, 4), limit_us=round(limit, 2), ok=bool(us[kind, J] <= limit))
                ok &= row["ok"]
                rows.append(row)
                print(f"{row['shape']:24s} img_{kind:5s} J={J}: {row['us']:8.2f} us   rgb_{kind:5s} {row['rgb_us']:8.2f} us   limit {row['limit_us']:8.2f}   "
                      f"{'ok' if row['ok'] else 'MISS'}")
    return rows, ok


def sweep_rows(a):
    """us of img_in / img_out (J = 4, C = 16, bf16) at sizes around the threshold, in THIS process' SGX_IMG1_MIN setting."""
    L = N.lib()
    out = {}
    for npix in (8192, 16384, 32768, 65536, 131072, 262144, 1048576, 4194304):
        ks = {k: v for k, v in kernels(L, npix, 16, torch.bfloat16).items() if k in (("in", 4), ("out", 4))}
        us = medians(ks, a.iters)
        out[str(npix)] = dict(img_in=round(us["in", 4], 2), img_out=round(us["out", 4], 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--commit", default=os.environ.get("SGX_COMMIT", ""))
    ap.add_argument("--out", default="")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert a.iters >= 20, "at least 20 timed launches per kernel"
    if a.sweep_child:
        print("SWEEP " + json.dumps(sweep_rows(a)))
        return 0
    out = dict(what="image-side 1x1 kernels (csrc/imgconv.hip) against the 3-channel kernels, one MI355X, one session", box=socket.gethostname(),
               commit=a.commit, iters=a.iters, method="interleaved launches, one event pair per launch on one stream, median")
    out["rows"], ok = judge(a)
    out["all_within_limits"] = ok
    if a.sweep:
        cols = {}
        for name, val in (("short_lived_from_65536", None), ("loop_only", "0")):
            env = dict(os.environ)
            if val is not None:
                env["SGX_IMG1_MIN"] = val
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sweep-child", "--iters", str(a.iters)], env=env, capture_output=True,
                               text=True, timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("SWEEP ")]
            if r.returncode != 0 or not line:
                print(r.stdout[-2000:], r.stderr[-2000:])
                return 1                                                     # (a failed child: nothing more is started on the GPU)
            cols[name] = json.loads(line[0][6:])
        out["threshold_sweep_J4_C16_bf16_us"] = cols
        for npix in cols["loop_only"]:
            lo, sh = cols["loop_only"][npix], cols["short_lived_from_65536"][npix]
            print(f"npix {int(npix):8d}: img_in loop {lo['img_in']:7.2f} / default {sh['img_in']:7.2f} us   img_out loop {lo['img_out']:7.2f} / default {sh['img_out']:7.2f} us")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
