"""Helpers the augmentation tests share (test_gpu_{diffaug,ada,blit,geom,color,filter,corrupt}.py and the *_cpu.py files of the
stages).  A helper lives here when its copies were the same in every file that had one; a file whose copy checks something else
keeps its own."""
import pytest
import torch

import ada_ref as A
import aug_ref as AR
from gpu_util import DEV, MID, load_into, mid_params

OPT = dict(learning_rate=0.003, beta_1=0, beta_2=0.99, eps=1e-8)


def dev_state(p):
    return torch.from_numpy(A.new_state(p)).to(DEV)


def on_device(t, off=0):
    buf = torch.zeros(t.numel() + off, device=DEV)
    v = buf[off:].view(t.shape)
    v.copy_(t.to(DEV))
    return v


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def bits_equal(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def recorded(fn):
    from stylegan.pytorch_amd import native as N
    N.prof_start(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    AR.assert_records_are_planned(N)                                        # every image-pass launch: a launch sgx_aug_plan reports for its call
    return out, [r[4].split(" ")[0] for r in N.prof_records()]


def small_dis_cpu(**kw):
    from stylegan.pytorch_amd.GAN import Discriminator
    return Discriminator(resolution=8, blur_filter=[1, 2, 1], fmap_base=64, fmap_max=16, **kw)


def small_dis(**kw):
    return small_dis_cpu(**kw).to(DEV)


def mid_dis(policy, **kw):
    from stylegan.pytorch_amd.GAN import Discriminator
    return Discriminator(resolution=MID["resolution"], num_channels=3, use_wscale=True, blur_filter=[1, 2, 1], fmap_base=MID["fmap_base"],
                         fmap_max=MID["fmap_max"], structure="linear", diffaug_policy=policy, **kw).to(DEV)


def load_ada(module, params):
    if getattr(module, "ada", False):
        params = dict(params, ada_state=module.ada_state.detach().clone())
    return load_into(module, params)


@pytest.fixture(scope="module")
def dparams():
    return mid_params(torch.float64)[1]


def make_sg(policy, use_graphs=False, data_parallel=None, **ada):
    from stylegan.pytorch_amd.GAN import StyleGAN
    return StyleGAN(structure="linear", resolution=128, num_channels=3, latent_size=512,
                    g_args=dict(latent_size=512, mapping_layers=MID["mapping_layers"], blur_filter=[1, 2, 1], truncation_psi=0.7,
                                truncation_cutoff=8, fmap_base=MID["fmap_base"], fmap_max=MID["fmap_max"]),
                    d_args=dict(use_wscale=True, blur_filter=[1, 2, 1], fmap_base=MID["fmap_base"], fmap_max=MID["fmap_max"],
                                diffaug_policy=policy, **ada),
                    g_opt_args=OPT, d_opt_args=OPT, loss="logistic", d_repeats=1, use_ema=True, ema_decay=0.999,
                    device=torch.device(DEV), use_graphs=use_graphs, data_parallel=data_parallel)
