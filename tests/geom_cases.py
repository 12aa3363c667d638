"""Pinned draws shared by tests/test_gpu_geom.py (the network test) and tests/test_geom_cpu.py (which checks on the CPU, on the
reference alone, that they mix what the network test needs mixed)."""
import torch

import blit_cases as C
import geom_ref as G

FULL8 = C.FULL + ",scale,rotate,aniso"
NET_B, NET_P = C.NET_B, C.NET_P


def spread_gates3(B):
    """[B,3] gate uniforms spread over (0, 1): at any p in steps of 0.2 from 0.1 some are below and some above."""
    return torch.tensor([[((3 * b + k) * 5 % 12 + 0.5) / 12 for k in range(3)] for b in range(B)], dtype=torch.float32)


def network_draws(depth):
    """-> (u [4,5] float32 array, gate uniforms [4,3] tensor, the per-image geometric bits they give at p = 0.5 under the full policy)."""
    u = G.edge_draws5(NET_B, seed=depth)
    gates = spread_gates3(NET_B)
    return u, gates, G.gates(gates.numpy(), NET_P, G.ALL).tolist()
