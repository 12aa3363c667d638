"""Pinned draws shared by tests/test_gpu_blit.py (the network test) and tests/test_blit_cpu.py (which checks on the CPU, on the
reference alone, that they mix what the network test needs mixed)."""
import torch

import blit_ref as Bl

FULL = "color,xflip,rot90,translation,cutout"
NET_B, NET_P = 4, 0.5


def spread_gates5(B):
    """[B,5] gate uniforms spread over (0, 1): at any p in steps of 0.2 from 0.1 some are below and some above."""
    return torch.tensor([[((3 * b + k) * 5 % 12 + 0.5) / 12 for k in range(5)] for b in range(B)], dtype=torch.float32)


def network_draws(depth):
    """-> (u [4,9] float32 array, gate uniforms [4,5] tensor, the per-image bits they give at p = 0.5 under the full policy)."""
    u = Bl.edge_draws9(NET_B, seed=depth)
    gates = spread_gates5(NET_B)
    return u, gates, Bl.gates_n(gates.numpy(), NET_P, Bl.ALL).tolist()
