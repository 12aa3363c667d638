#!/usr/bin/env python3
"""Generate channels.npz by EXECUTING THE REFERENCE on CPU for models that are not RGB: num_channels 1 and 4.

Same shims as make_golden.py (stub ``data`` module, no bytecode, float Adam betas); nothing from the reference is copied, only inputs
and outputs are written.  Runs only where the reference checkout exists (never on the GPU box, never in tests).

Two network configurations at resolution 16, 2 mapping layers, structure 'linear':
  a: fmap_base=64,  fmap_max=16  -- 16, 16, 8 feature maps at 4x4, 8x8, 16x16
  b: fmap_base=128, fmap_max=16  -- 16 everywhere: the widths the MFMA convolutions take (multiples of 16), so the HIP path can be
                                    held to these records at depth 2 as well
Per configuration and num_channels in {1, 4}: the state dict (names, shapes, [sum, sum|.|, norm] per tensor -- the values themselves are
golden_util.fill_value of the name, as in every fixture here, and would be megabytes of mapping weights), the pinned latents and noises,
generator images and discriminator scores at depth 0 and at depth 2 with alpha = 0.5, in fp32 and fp64; the conditional case
(num_channels=1, n_classes=3) likewise.  For configuration b: one LogisticGAN D step and G step at depth 2, alpha = 0.5 (losses,
gradients, updated parameters) as make_golden.py records them for the MID size.

    python tests/golden/make_golden_channels.py
"""
import os
import random
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/
sys.path.insert(0, os.environ.get("STYLEGAN_REFERENCE", "/root/reference"))
_d = types.ModuleType("data"); _d.get_data_loader = None; sys.modules["data"] = _d

import numpy as np  # noqa: E402
import torch  # noqa: E402

import golden_util as gu  # noqa: E402
from models import CustomLayers as CL  # noqa: E402
from models.GAN import Discriminator, Generator, StyleGAN  # noqa: E402

torch.set_num_threads(8)

RES, DEPTHS, B, NCLS = 16, 3, 4, 3
CONFIGS = {"a": dict(fmap_base=64, fmap_max=16), "b": dict(fmap_base=128, fmap_max=16)}
CASES = [(0, 1.0), (2, 0.5)]
TAGS = [("f32", torch.float32), ("f64", torch.float64)]
LABELS = torch.tensor([0, 2, 1, 2])


def g_kw(cfg, nc):
    return dict(num_channels=nc, latent_size=512, mapping_layers=2, blur_filter=[1, 2, 1], truncation_psi=0.7, truncation_cutoff=8, **cfg)


def d_kw(cfg):
    return dict(use_wscale=True, blur_filter=[1, 2, 1], **cfg)


def fill_module(m, dtype):
    sd = m.state_dict()
    m.load_state_dict({k: v if k.endswith(".kernel") else gu.fill_value(k, v.shape, dtype) for k, v in sd.items()})
    return m


def pin_noise(gen, dtype):
    mods = [m for m in gen.modules() if isinstance(m, CL.NoiseLayer)]
    for i, m in enumerate(mods):
        r = 4 * 2 ** (i // 2)
        m.noise = gu.seeded((B, 1, r, r), 100 + i, dtype)
    return mods


def record_state(out, pre, mod):
    sd = {k: v for k, v in mod.state_dict().items() if not k.endswith(".kernel")}
    names = sorted(sd)
    out[pre + "names"] = np.array(names)
    out[pre + "shapes"] = np.array([";".join(str(int(s)) for s in sd[k].shape) for k in names])
    out[pre + "stats"] = np.array([gu.tensor_stats(sd[k]) for k in names])


def forwards(out, ck, cfg):
    for nc, cond in ((1, False), (4, False), (1, True)):
        key = f"{ck}_{'cond' if cond else 'nc'}{nc}_"
        for tag, dtype in TAGS:
            extra = dict(conditional=True, n_classes=NCLS) if cond else {}
            gen = Generator(resolution=RES, structure="linear", **g_kw(cfg, nc), **extra)
            dis = Discriminator(resolution=RES, num_channels=nc, structure="linear", **d_kw(cfg), **extra)
            if dtype == torch.float64:
                gen.double(); dis.double()
            fill_module(gen, dtype); fill_module(dis, dtype)
            gen.train(); dis.train()
            pin_noise(gen, dtype)
            gen.style_mixing_prob = None
            if tag == "f32":
                record_state(out, key + "g_", gen); record_state(out, key + "d_", dis)
            z = gu.seeded((B, 512), 11, dtype)
            labels = LABELS if cond else None
            for depth, alpha in CASES:
                gen.truncation.avg_latent.copy_(gu.fill_value("truncation.avg_latent", (512,), dtype))
                r = 4 * 2 ** depth
                real = gu.seeded((B, nc, r, r), 60 + depth, dtype)
                with torch.no_grad():
                    out[f"{key}{tag}_g_d{depth}_img"] = gen(z, depth, alpha, labels_in=labels) if cond else gen(z, depth, alpha)
                    out[f"{key}{tag}_d_d{depth}_score"] = dis(real, depth, alpha, labels_in=labels) if cond else dis(real, depth, alpha)


def steps(out, ck, cfg):
    depth, alpha = 2, 0.5
    opt = dict(learning_rate=0.003, beta_1=0.0, beta_2=0.99, eps=1e-8)
    for nc in (1, 4):
        key = f"{ck}_step{nc}_"
        grads = {}
        for tag, dtype in TAGS:
            torch.manual_seed(0)
            gk = {k: v for k, v in g_kw(cfg, nc).items() if k != "num_channels"}
            sg = StyleGAN(structure="linear", resolution=RES, num_channels=nc, latent_size=512, g_args=gk, d_args=d_kw(cfg), g_opt_args=opt,
                          d_opt_args=opt, loss="logistic", d_repeats=1, use_ema=True, ema_decay=0.999, device=torch.device("cpu"))
            if dtype == torch.float64:
                sg.gen.double(); sg.dis.double(); sg.gen_shadow.double()
            fill_module(sg.gen, dtype); fill_module(sg.dis, dtype)
            sg.gen_shadow.load_state_dict(sg.gen.state_dict())
            sg.gen.train(); sg.dis.train(); sg.gen_shadow.train()
            pin_noise(sg.gen, dtype)
            z = gu.seeded((B, 512), 21, dtype); real = gu.seeded((B, nc, RES, RES), 22, dtype)
            _randn = torch.randn
            if dtype == torch.float64:
                torch.randn = lambda *a, **k: _randn(*a, **k).double()     # latents2 (models/GAN.py:282): same values, widened
            torch.manual_seed(77); random.seed(77)
            out[f"{key}{tag}_d_loss"] = sg.optimize_discriminator(z, real, depth, alpha)
            grads[tag, "d"] = {k: p.grad.clone().double() for k, p in sg.dis.named_parameters() if p.grad is not None}
            torch.manual_seed(78); random.seed(78)
            out[f"{key}{tag}_g_loss"] = sg.optimize_generator(z, real, depth, alpha)
            torch.randn = _randn
            grads[tag, "g"] = {k: p.grad.clone().double() for k, p in sg.gen.named_parameters() if p.grad is not None}
            out[f"{key}{tag}_avg_latent"] = sg.gen.truncation.avg_latent
            for net, mod in (("d", sg.dis), ("g", sg.gen), ("s", sg.gen_shadow)):
                sd = dict(mod.named_parameters())
                names = sorted(sd)
                out[f"{key}{net}_param_names"] = np.array(names)
                out[f"{key}{tag}_{net}_param_stats"] = np.array([gu.tensor_stats(sd[k]) for k in names])
                for k in names:                                            # full tensors: the fp64 run's, the small ones, not the shadow's
                    if tag == "f64" and net != "s" and sd[k].numel() <= 1024:
                        out[f"{key}{net}_param64::{k}"] = sd[k]
        for net in ("d", "g"):
            names = sorted(grads["f64", net])
            out[f"{key}{net}_grad_names"] = np.array(names)
            out[f"{key}{net}_grad_norm64"] = np.array([float(torch.linalg.vector_norm(grads["f64", net][k])) for k in names])
            out[f"{key}{net}_grad_err32"] = np.array([float(torch.linalg.vector_norm(grads["f32", net][k] - grads["f64", net][k])) for k in names])
            for k in names:
                if grads["f64", net][k].numel() <= 1024:
                    out[f"{key}{net}_grad64::{k}"] = grads["f64", net][k]


if __name__ == "__main__":
    out = {}
    for ck, cfg in CONFIGS.items():
        forwards(out, ck, cfg)
    steps(out, "b", CONFIGS["b"])                                          # (the configuration both the oracle and the HIP path run)
    out["z"] = gu.seeded((B, 512), 11); out["z_step"] = gu.seeded((B, 512), 21); out["labels"] = LABELS
    for i in range(2 * DEPTHS):
        out[f"noise{i}"] = gu.seeded((B, 1, 4 * 2 ** (i // 2), 4 * 2 ** (i // 2)), 100 + i)
    arrs = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, "channels.npz"), **arrs)
    print("wrote channels.npz", len(arrs), "arrays")
