"""Shared by tests/test_channels_cpu.py and tests/test_gpu_channels.py: the small networks of tests/golden/channels.npz (resolution 16,
2 mapping layers, num_channels 1 / 4, optionally conditional) as oracle parameter dicts, their pinned inputs, and the fixture itself."""
import os

import numpy as np
import torch

import golden_util as gu
from oracle import stylegan_oracle as O

RES, TOTAL_DEPTH, B, NCLS, MAPPING = 16, 3, 4, 3, 2
CONFIGS = {"a": dict(fmap_base=64, fmap_max=16), "b": dict(fmap_base=128, fmap_max=16)}      # tests/golden/make_golden_channels.py
CASES = [(0, 1.0), (2, 0.5)]


def fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "channels.npz"))


def params(cfg, nc, cond=False, dtype=torch.float64):
    """(generator params, discriminator params) in the oracle's functional form, reference state_dict keys, values from
    golden_util.fill_value.  The oracle's make_* helpers build the RGB shapes; the image-side tensors are re-shaped here."""
    gp = O.make_generator_params(RES, MAPPING, 1024 if cond else 512, cfg["fmap_base"], cfg["fmap_max"], dtype=dtype)
    dp = O.make_discriminator_params(RES, cfg["fmap_base"], cfg["fmap_max"], dtype=dtype)
    shapes_g = {k: tuple(v.shape) for k, v in gp.items()}
    shapes_d = {k: tuple(v.shape) for k, v in dp.items()}
    jd = 2 * nc if cond else nc
    for k, s in shapes_g.items():
        if ".to_rgb." in k:
            shapes_g[k] = (nc,) + s[1:] if k.endswith("weight") else (nc,)
    for k, s in shapes_d.items():
        if k.startswith("from_rgb.") and k.endswith("weight"):
            shapes_d[k] = (s[0], jd, 1, 1)
    if cond:
        shapes_g["class_embedding.weight"] = (NCLS, 512)
        for i in range(TOTAL_DEPTH):                                      # embeddings[i]: resolution RES / 2^i (the last one 4x4)
            r = RES >> i
            shapes_d[f"embeddings.{i}.weight"] = (NCLS, nc * r * r)
    out = []
    for shapes, src in ((shapes_g, gp), (shapes_d, dp)):
        p = {}
        for k, s in shapes.items():
            rg = src[k].requires_grad if k in src else True
            p[k] = gu.fill_value(k, s, dtype).requires_grad_(rg)
        out.append(p)
    return out[0], out[1]


def noises(dtype=torch.float64):
    return [gu.seeded((B, 1, 4 * 2 ** (i // 2), 4 * 2 ** (i // 2)), 100 + i, dtype) for i in range(2 * TOTAL_DEPTH)]


def real_for(nc, depth, dtype=torch.float64):
    r = 4 * 2 ** depth
    return gu.seeded((B, nc, r, r), 60 + depth, dtype)


def labels():
    return torch.tensor([0, 2, 1, 2])


def oracle_forward(gp, dp, nc, depth, alpha, cond, dtype):
    """(generator image, discriminator score of the pinned real batch) as the fixture's forwards() computes them."""
    z = gu.seeded((B, 512), 11, dtype)
    lab = labels() if cond else None
    gp = dict(gp)
    gp["truncation.avg_latent"] = gu.fill_value("truncation.avg_latent", (512,), dtype)
    with torch.no_grad():
        img, _ = O.generator(gp, z, depth, alpha, noises(dtype), mapping_layers=MAPPING, num_layers=2 * TOTAL_DEPTH, labels=lab)
        score = O.discriminator(dp, real_for(nc, depth, dtype), depth, alpha, TOTAL_DEPTH, labels=lab)
    return img, score
