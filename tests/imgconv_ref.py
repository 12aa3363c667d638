"""fp64 restatements of the image-side 1x1 kernels of csrc/imgconv.hip and of the J-channel uint8 ingest, written from their definitions in
include/sgx.h.  Test-side only; nothing here calls the library under test.

Every reference takes fp64 tensors and returns ``(ref, S, n)``: the value, the same expression on the absolute values of inputs and
coefficients (the per-element scale of the fp32 arithmetic error), and the length of the longest fp32 chain the kernel runs for one output
element -- what ``streaming_ref.assert_elementwise(got, ref, S, n, dtype)`` takes.  The weight is the flat parameter, element (j, c) at
``w[j*sj + c*sc]``."""
import math

import torch

WGRAD_BLOCKS = 1024                 # csrc/imgconv.hip IMG_WGRAD_BLOCKS


def ve(dtype):
    """Elements of one 16-byte vector of the activation dtype."""
    return 4 if dtype == torch.float32 else 8


def layout(kind, J, C):
    """(sj, sc) of the parameter: 'in' = from_rgb [C][J][1][1], 'out' = to_rgb [J][C][1][1]."""
    return (1, J) if kind == "in" else (C, 1)


def weight(w, J, sj, sc, C):
    """W(j, c) = w[j*sj + c*sc] as a [J][C] view of the flat parameter."""
    return torch.as_strided(w, (J, C), (sj, sc))


def img_in(img, w, J, sj, sc, wscale, bias, C):
    """y[p][c] = bias[c] + sum_j img[p][j] * (wscale * W(j, c)).  Chain: wscale * w, the product, J - 1 sums, the bias."""
    W = wscale * weight(w, J, sj, sc, C)
    ref, S = img @ W, img.abs() @ W.abs()
    if bias is not None:
        ref, S = ref + bias, S + bias.abs()
    return ref, S, 2 + J


def img_out(x, w, J, sj, sc, wscale, bias, C, dtype):
    """img[p][j] = bias[j] + sum_c x[p][c] * (wscale * W(j, c)).  Chain: wscale * w, the product, a lane's VE * ceil(cv / lpp) sums,
    log2(lpp) exchange steps, the bias (lpp = min(C / VE, 16) lanes per pixel)."""
    W = wscale * weight(w, J, sj, sc, C)
    ref, S = x @ W.t(), x.abs() @ W.abs().t()
    if bias is not None:
        ref, S = ref + bias, S + bias.abs()
    cv = C // ve(dtype)
    lpp = min(cv, 16)
    return ref, S, 2 + ve(dtype) * math.ceil(cv / lpp) + int(math.log2(lpp)) + 1


def img_wgrad(img, f, J, sj, sc, wscale, C, dtype):
    """dw[j*sj + c*sc] = wscale * sum_p img[p][j] * f[p][c] in the flat parameter layout (J * C values).  Chain: the product, then a
    lane's fp32 partial over ceil(per / rows) pixels (per = ceil(npix / blocks), rows = 256 / (C / VE)); everything after is fp64."""
    npix = img.shape[0]
    g, ga = wscale * (img.t() @ f), abs(wscale) * (img.abs().t() @ f.abs())             # [J][C]
    ref = torch.zeros(J * C, dtype=f.dtype, device=f.device)
    S = torch.zeros_like(ref)
    weight(ref, J, sj, sc, C).copy_(g)
    weight(S, J, sj, sc, C).copy_(ga)
    nblk = max(1, min(WGRAD_BLOCKS, (npix + 63) // 64))
    per = (npix + nblk - 1) // nblk
    rows = 256 // (C // ve(dtype))
    return ref, S, 1 + max(1, math.ceil(per / rows))


def images_u8(src, flip, chw):
    """(v / 255 - 0.5) / 0.5 per byte, NHWC out; flip[b] mirrors image b.  src: uint8 [B][H][W][J] or [B][J][H][W].  Chain: the division
    and the subtraction (x 2 is exact)."""
    v = src.to(torch.float64)
    if chw:
        v = v.permute(0, 2, 3, 1)
    if flip is not None:
        v = torch.where(torch.as_tensor(flip).to(v.device).bool().view(-1, 1, 1, 1), v.flip(2), v)
    v = v.contiguous()
    return (v / 255.0 - 0.5) / 0.5, (v / 255.0 + 0.5) / 0.5, 2
