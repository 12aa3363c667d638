"""Pinned draws shared by tests/test_gpu_color.py (the network test) and tests/test_color_cpu.py (which checks on the CPU, on the
reference alone, that they mix what the network test needs mixed)."""
import torch

import color_ref as K
import geom_cases as GC

FULL13 = GC.FULL8 + "," + ",".join(K.OPS)
NET_B, NET_P = GC.NET_B, GC.NET_P


def network_gates5():
    """[4,5] gate uniforms for p = 0.5: image 0 has all five ops off, image 3 all five on, images 1 and 2 split them
    (brightness, lumaflip, saturation / contrast, hue)."""
    on, off = 0.25, 0.75
    return torch.tensor([[off, off, off, off, off], [on, off, on, off, on], [off, on, off, on, off], [on, on, on, on, on]], dtype=torch.float32)


def network_draws(depth):
    """-> (u [4,8] float32 array, gate uniforms [4,5] tensor, the per-image colour bits they give at p = 0.5 under the full policy)."""
    u = K.edge_draws8(NET_B, seed=depth)
    gates = network_gates5()
    return u, gates, K.gates(gates.numpy(), NET_P, K.ALL).tolist()
