"""CPU side of tests/test_gpu_streaming_kernels.py: (1) every hipLaunchKernelGGL site of csrc/pointwise.hip and of csrc/small.hip is claimed by
a row of streaming_ref.CASES or excused by name with a reason, so a kernel added later fails here until it gets a case; (2) the helper's own
criterion passes honest fp32-computed, once-rounded results and fails planted errors that the suite's rel-L2 metric lets through."""
import collections
import os
import re

import numpy as np
import pytest
import torch

import gpu_util
import small_ref as SM
import streaming_ref as SR
from oracle import stylegan_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stylegan", "pytorch_amd", "csrc")
SITE = re.compile(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_][A-Za-z_0-9]*)\s*(<[^>()]*>)?")
LITERAL = re.compile(r"^(-?\d+|true|false|float|bf16_t)$")

# Kernels of small.hip that are not streaming kernels are claimed by the rows of tests/small_ref.py, site by site and instantiation by
# instantiation (tests/test_gpu_small_paths.py runs them; the loss head's older rel-L2 test is in tests/test_gpu_fusions.py).  The scan below takes
# those rows beside streaming_ref's.
BY_INT = re.compile(r"sgx_by_int<([^<>()]*)>\(")
# Rows per entry point.  A row is a launch path someone decided to cover: dropping one has to be a decision made here too.
ROWS = {"sgx_bias_act": 10, "sgx_lrelu_bwd": 7, "sgx_lrelu_bwd_bits": 3, "sgx_axpby": 11, "sgx_axpby_dev": 10, "sgx_blur3x3_act": 43, "sgx_blur3x3_bits": 8,
        "sgx_blur_kxk": 18, "sgx_pool2": 10, "sgx_up2": 10, "sgx_up2_add": 7, "sgx_downsample_fade_rgb": 3, "sgx_images_u8_to_nhwc": 8, "sgx_colsum": 16,
        "sgx_rgb_in": 18, "sgx_rgb_in_add": 5, "sgx_rgb_out": 26, "sgx_rgb_out_fade": 6, "sgx_rgb_wgrad": 15, "sgx_fade_rgb_bwd2": 1, "sgx_fade_rgb_bwd": 3, "sgx_rgb_out_epi": 2, "sgx_rgb_wgrad_epi": 2,
        "sgx_sumsq_f32": 3, "sgx_scale_dev_f32": 5, "sgx_pixelnorm_fwd": 3, "sgx_pixelnorm_bwd": 3}
# ... and rejection rows per entry point (streaming_ref.REJECTIONS)
REJECTION_ROWS = {"sgx_bias_act": 2, "sgx_blur_kxk": 1, "sgx_colsum": 2, "sgx_rgb_wgrad": 1, "sgx_rgb_out": 2, "sgx_pool2": 1, "sgx_up2": 1, "sgx_up2_add": 1,
                  "sgx_rgb_in": 1, "sgx_lrelu_bwd_bits": 1, "sgx_img_in": 1}


def launch_sites(path):
    with open(path) as f:
        src = f.read()
    src = re.sub(r"#define hipLaunchKernelGGL.*", "", src)
    out = []
    for m in SITE.finditer(src):
        by = by_int_params(src, m.start())
        out.append((m.group(1), (m.group(2) or "").strip()) + ((by,) if by else ()))
    return out


def by_int_params(src, at):
    """The compile-time integers a site at src[at] may be instantiated with: {name: the listed values} for the parameter of the
    sgx_by_int<a, b, ...>(j, [&](auto p) { constexpr int NAME = p(); ... }) call that encloses it (p() itself and every NAME it is given), read
    from the text between the call and the site; {} where no such call is still open there."""
    for b in reversed(list(BY_INT.finditer(src, 0, at))):
        between = re.sub(r"//.*", "", src[b.end():at])
        if between.count("(") - between.count(")") < 0:      # that call was closed before the site
            continue
        p = re.search(r"\(\s*auto\s+(\w+)\s*\)", between)
        if not p:
            return {}
        values = [v.strip() for v in b.group(1).split(",")]
        names = [p.group(1) + "()"] + re.findall(r"constexpr\s+int\s+(\w+)\s*=\s*" + p.group(1) + r"\(\)\s*;", between)
        return {n: values for n in names}
    return {}


def split_args(targs):
    return [a.strip() for a in targs[1:-1].split(",")] if targs else []


def claims(site, kernel):
    """Does a case's kernel instantiation answer this launch site?  Same template, and every argument the site spells as a literal agrees
    (an argument that is a template parameter or constant of the launcher -- T, ROWS, PF -- is left to the row)."""
    m = re.match(r"^([A-Za-z_0-9]+)(<.*>)?$", kernel)
    if m.group(1) != site[0]:
        return False
    sa, ka = split_args(site[1]), split_args(m.group(2) or "")
    if len(sa) != len(ka) and not (len(sa) < len(ka)):      # (defaulted trailing arguments: blur3x3s_kernel's NT)
        return False
    return all(not LITERAL.match(s) or s == k for s, k in zip(sa, ka))


def unclaimed(sites, cases, excluded):
    kernels = {k for c in cases for k in c.kernels}
    miss = []
    for site in sites:
        text = site[0] + site[1]
        if text in excluded:
            continue
        mine = [k for k in kernels if claims(site, k)]
        if not mine:
            miss.append(text)
            continue
        if "T" in split_args(site[1]):                      # a site generic in the dtype: both dtypes where both exist (kernel modes 4 / 5 are bf16 only)
            need = {"bf16_t"} if any(a in ("4", "5") for a in split_args(site[1])[1:2]) and site[0].startswith("blur3x3") else {"float", "bf16_t"}
            have = {split_args(re.match(r"^[A-Za-z_0-9]+(<.*>)$", k).group(1))[0] for k in mine}
            if not need <= have:
                miss.append(f"{text} for {sorted(need - have)}")
        for i, a in enumerate(split_args(site[1])):         # ... generic in the parameter of an enclosing sgx_by_int<a, b, ...>: every listed value
            values = (site[2] if len(site) > 2 else {}).get(a)
            if values:
                have = {split_args(re.match(r"^[A-Za-z_0-9]+(<.*>)$", k).group(1))[i] for k in mine}
                if not set(values) <= have:
                    miss.append(f"{text} for {[int(v) for v in values if v not in have]}")
    return miss


def all_sites():
    return launch_sites(os.path.join(CSRC, "pointwise.hip")), launch_sites(os.path.join(CSRC, "small.hip"))


def test_every_launch_site_is_claimed_or_excused():
    pw, sm = all_sites()
    # the scan found the launchers: every site of the two files.  small.hip has one site per kernel: pixelnorm 2, mbstd 3 (<T>), the GEMM's
    # outer-product, tile (<U> of sgx_by_int<1, 8>) and reduce kernels 3, the style affines 3 (<MB> of sgx_by_int<4, 8, 16, 32>), sumsq 2,
    # the logistic head 1, scale_dev 1
    assert len(pw) == 52 and len(sm) == 15, (len(pw), len(sm))
    assert unclaimed(pw, SR.CASES, SR.EXCLUDED_SITES) == []
    assert unclaimed(sm, SR.CASES + SM.CASES, SR.EXCLUDED_SITES) == []
    assert unclaimed(sm, SR.CASES, SR.EXCLUDED_SITES) != []                                     # ... a claim by the rows, no longer an excuse by name
    # a site generic in an sgx_by_int parameter needs a row for each listed value: the lists are read, and dropping the rows of one value is noticed
    by = {s[0]: s[2] for s in sm if len(s) > 2}
    assert by == {"gemm_f32_kernel": {"u()": ["1", "8"], "U": ["1", "8"]},
                  **{f"style_{e}_kernel": {"mb()": ["4", "8", "16", "32"], "MB": ["4", "8", "16", "32"]} for e in ("fwd", "bwd_data", "bwd_param")}}, by
    no_k8 = [c for c in SM.CASES if SM.K8 not in c.kernels]
    assert unclaimed(sm, SR.CASES + no_k8, SR.EXCLUDED_SITES) == ["gemm_f32_kernel<U> for [8]"]
    no_mb16 = [c for c in SM.CASES if not (c.entry == "sgx_style_fwd" and SM.style_mb(c.args["B"]) == 16)]
    assert unclaimed(sm, SR.CASES + no_mb16, SR.EXCLUDED_SITES) == ["style_fwd_kernel<MB> for [16]"]
    # the excuses name sites that exist, the covered small.hip kernels are there, and every reason is written down
    texts = {s[0] + s[1] for s in pw + sm}
    assert set(SR.EXCLUDED_SITES) <= texts, set(SR.EXCLUDED_SITES) - texts
    assert set(SR.SMALL_HIP_COVERED) <= {s[0] for s in sm}
    assert all(len(r) > 10 for r in list(SR.EXCLUDED_SITES.values()) + list(SR.EXCLUDED_PATHS.values()))
    # and every kernel a row names is launched somewhere in the two files
    for c in SR.CASES:
        for k in c.kernels:
            assert any(claims(s, k) for s in pw + sm), (c.id, k)
        assert c.why and c.entry in ROWS, c.id


def test_a_new_kernel_or_a_dropped_row_is_noticed():
    pw, _ = all_sites()
    assert unclaimed(pw + [("brand_new_kernel", "<float>")], SR.CASES, SR.EXCLUDED_SITES) == ["brand_new_kernel<float>"]
    assert unclaimed(pw + [("blur3x3_kernel", "<T, 6, ROWS>")], SR.CASES, SR.EXCLUDED_SITES) == ["blur3x3_kernel<T, 6, ROWS>"]
    without = [c for c in SR.CASES if c.id != "pool2-f32-rgb-W16" and c.id != "pool2-f32-rgb-W1024"]
    assert unclaimed(pw, without, SR.EXCLUDED_SITES) == ["pool2_rgb_kernel"]
    no_bf16_m3 = [c for c in SR.CASES if not c.kernels[0].startswith("blur3x3_kernel<bf16_t, 3,")]
    assert unclaimed(pw, no_bf16_m3, SR.EXCLUDED_SITES) == ["blur3x3_kernel<T, 3, ROWS> for ['bf16_t']"]
    assert dict(collections.Counter(c.entry for c in SR.CASES)) == ROWS
    assert dict(collections.Counter(r[1] for r in SR.REJECTIONS)) == REJECTION_ROWS
    assert len({r[0] for r in SR.REJECTIONS}) == len(SR.REJECTIONS)


def test_case_table_shapes_select_what_they_say():
    """The launcher rules of csrc/pointwise.hip restated on the table's own arguments: thresholds sit where the rows say."""
    by = {c.id: c for c in SR.CASES}
    for c in SR.CASES:
        a, ve = c.args, (4 if c.dtype == torch.float32 else 8)
        if c.entry.startswith("sgx_blur3x3"):
            cv = a["C"] // ve
            lanes8 = a["B"] * ((a["H"] + 7) // 8) * a["W"] * cv
            km = int(SR_args(c.kernels[0])[1])
            if lanes8 < SR.BLUR_LANES8:
                want = "2>"
            elif km != 3 and cv <= 16 and cv & (cv - 1) == 0 and (a["W"] * cv) % 64 == 0:
                want = "false>"
            else:
                want = "8>"
            assert c.kernels[0].endswith(want), (c.id, lanes8, cv)
        if c.entry in ("sgx_rgb_in", "sgx_rgb_in_add"):
            nvec = a["npix"] * (a["C"] // ve)
            assert c.kernels[0].startswith("rgb_in1_kernel") == (nvec >= 65536 and a["C"] <= 2048), c.id
        if c.entry in ("sgx_rgb_out", "sgx_rgb_out_fade"):
            npix = a["npix"] if "npix" in a else a["B"] * a["H"] * a["W"]
            assert c.kernels[0].startswith("rgb_out1_kernel") == (npix >= 65536 and a["C"] // ve <= 16), c.id
    assert by["blur-bf16-m0-below-lanes8"].args["H"] == 1012 and by["rgb_in-bf16-65535"].args["npix"] == 65535
    big = [c for c in SR.CASES if c.id.endswith("headline")]
    assert len(big) >= 14 and all(c.dtype == torch.bfloat16 for c in big)


def SR_args(kernel):
    return split_args(re.match(r"^[A-Za-z_0-9]+(<.*>)$", kernel).group(1))


# ---------------------------------------------------------------------------------------------------------------- the helper on CPU tensors
def _seeded(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _axpby_emulated():
    a, b = _seeded((2, 256, 256, 16), 1, torch.bfloat16), _seeded((2, 256, 256, 16), 2, torch.bfloat16)
    al, be = SR.f32(0.3), SR.f32(0.7)
    got = (torch.tensor(al) * a.float() + torch.tensor(be) * b.float()).bfloat16()      # fp32 compute, one rounding
    ref, S = SR.axpby(a.double(), b.double(), al, be)
    return got, ref, S


def test_elementwise_criterion_passes_fp32_emulations():
    got, ref, S = _axpby_emulated()
    assert SR.assert_elementwise(got, ref, S, 2, torch.bfloat16, "axpby") <= 1.0
    # rgb_in: wscale * w, three products, two sums, the bias -- in fp32, stored as bf16 and as fp32
    C, npix, ws = 24, 4099, SR.f32(0.37)
    img, w, bias = _seeded((npix, 3), 3), _seeded((3 * C,), 4), _seeded((C,), 5)
    for sj, sc in ((1, 3), (C, 1)):
        W = torch.tensor(ws) * SR.rgb_weight(w, sj, sc, C)
        v = bias + ((img[:, 0:1] * W[0] + img[:, 1:2] * W[1]) + img[:, 2:3] * W[2])
        ref, S = SR.rgb_in(img.double(), w.double(), sj, sc, ws, bias.double(), C)
        assert torch.allclose(ref, img.double() @ (ws * SR.rgb_weight(w, sj, sc, C).double()) + bias.double())
        SR.assert_elementwise(v.bfloat16(), ref, S, 5, torch.bfloat16, "rgb_in bf16")
        SR.assert_elementwise(v, ref, S, 5, torch.float32, "rgb_in fp32")
    # the blur, all four modes, against the oracle's statement of the filter too
    x, z = _seeded((2, 9, 7, 16), 6, torch.bfloat16), _seeded((2, 9, 7, 16), 7, torch.bfloat16)
    assert torch.allclose(SR._blur121(x.double()), O.blur3(x.double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1), rtol=1e-13, atol=1e-15)
    for mode in range(4):
        xf, sl = x.float(), torch.where(z.float() > 0, 1.0, SR.LRELU).float()
        pre = torch.where(xf > 0, xf, torch.tensor(SR.LRELU) * xf) if mode == 1 else (xf * sl if mode == 3 else xf)
        got = SR._blur121(pre)                                  # fp32 throughout
        assert got.dtype == torch.float32
        if mode == 2:
            got = got * sl
        ref, S = SR.blur3x3(x.double(), z.double(), mode)
        SR.assert_elementwise(got.bfloat16(), ref, S, 9 + (1 if mode else 0), torch.bfloat16, f"blur mode {mode}")
        rb, Sb = SR.blur3x3(x.double(), z > 0, mode)
        assert torch.equal(rb, ref) and torch.equal(Sb, S)
    # sign bits round-trip in the library's layout
    m = _seeded((5, 3, 24), 8) > 0
    assert torch.equal(SR.unpack_bits(SR.pack_bits(m), 24), m) and SR.pack_bits(m).shape == (5, 3, 3)
    assert int(SR.pack_bits(torch.tensor([[True] + [False] * 6 + [True]]))[0, 0]) == 0x81


def test_elementwise_criterion_fails_planted_errors_the_rel_l2_metric_passes():
    got, ref, S = _axpby_emulated()
    # (1) the last 16-byte vector zeroed: a tail that did not run.  rel-L2 moves by ~2e-3: under the suite's bf16 tolerances (3e-3 .. 6e-3)
    tail = got.clone(); tail.view(-1)[-8:] = 0
    gpu_util.assert_close(tail.float(), ref, 3e-3, "zeroed tail vs the suite's metric")
    assert gpu_util.rel_err(tail.float(), ref) > gpu_util.rel_err(got.float(), ref)
    with pytest.raises(AssertionError, match=r"8 of 2097152 elements.*flat index 2097144 \(1, 255, 255, 8\)"):
        SR.assert_elementwise(tail, ref, S, 2, torch.bfloat16, "zeroed tail")
    # (2) one element 2 bf16 ulps off
    off = got.clone()
    i = int((got.view(-1).float().abs() > 0.5).nonzero()[0])
    off.view(-1).view(torch.int16)[i] += 2
    gpu_util.assert_close(off.float(), ref, 3e-3, "2 ulps")
    with pytest.raises(AssertionError, match=rf"1 of 2097152 elements.*flat index {i} "):
        SR.assert_elementwise(off, ref, S, 2, torch.bfloat16, "2 ulps")
    # (3) a NaN (an unwritten sentinel: every byte SENTINEL) -- `err > bound` would be False for it
    nan = got.clone()
    nan.view(-1).view(torch.uint8)[2 * 77:2 * 78] = SR.SENTINEL
    assert bool(nan.view(-1)[77].isnan())
    with pytest.raises(AssertionError, match=r"1 of 2097152 elements.*flat index 77 \(0, 0, 4, 13\)"):
        SR.assert_elementwise(nan, ref, S, 2, torch.bfloat16, "nan")
    f = torch.full((3,), float("nan"))
    f.view(torch.uint8)[:] = SR.SENTINEL
    assert bool(f.isnan().all())
    with pytest.raises(AssertionError):
        SR.assert_elementwise(f, torch.zeros(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64), 100, torch.float32, "fp32 sentinel")


@pytest.mark.parametrize("dtype,shift", [(torch.float32, 0), (torch.bfloat16, 0), (torch.float32, 4)])
def test_guard_bands_catch_a_planted_overwrite(dtype, shift):
    g = SR.Guarded((3, 5, 7), dtype, "cpu", shift)
    assert g.t.shape == (3, 5, 7) and g.t.is_contiguous() and bool(g.t.isnan().all())
    assert g.lo >= SR.GUARD and g.buf.numel() - g.lo - g.nbytes >= SR.GUARD
    assert (g.t.data_ptr() - g.buf.data_ptr()) % 256 == shift
    g.t.zero_()
    g.assert_intact("clean")
    g.buf[g.lo + g.nbytes] = 0                                 # one byte past the end
    with pytest.raises(AssertionError, match="back guard band overwritten, first at byte 0 "):
        g.assert_intact("overrun")
    g.buf[g.lo + g.nbytes] = SR.SENTINEL
    g.buf[g.lo - 3] = 1
    with pytest.raises(AssertionError, match="front guard band overwritten, first at byte -3 "):
        g.assert_intact("underrun")


def test_kernel_id_and_references_on_tiny_inputs():
    assert SR.kernel_id("void blur3x3s_kernel<unsigned short, 0, 8, 3, false>(unsigned short const*, unsigned short const*, unsigned short*, int)") == \
        "blur3x3s_kernel<bf16_t, 0, 8, 3, false>"
    assert SR.kernel_id("pool2_rgb_kernel(float const*, float*, int, int, int, float)") == "pool2_rgb_kernel"
    x = torch.arange(2 * 4 * 4 * 3, dtype=torch.float64).view(2, 4, 4, 3)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    assert torch.equal(nchw(SR.up2(x, 1.0)[0]), O.upscale2d(nchw(x)))
    assert torch.allclose(nchw(SR.pool2(x, 0.25)[0]), O.downscale2d(nchw(x)))
    u8 = ((torch.arange(2 * 4 * 8 * 3) * 89 + 3) % 256).to(torch.uint8).view(2, 4, 8, 3)
    flip = torch.tensor([1, 0], dtype=torch.int32)
    want = O.images_u8_to_float(u8, [True, False]).permute(0, 2, 3, 1).double()
    assert torch.allclose(SR.images_u8(u8, flip, 0)[0], want, atol=1e-6)
    assert torch.allclose(SR.images_u8(u8.permute(0, 3, 1, 2).contiguous(), flip, 1)[0], want, atol=1e-6)
    v = _seeded((5, 70), 9).double()
    assert torch.allclose(SR.pixelnorm_fwd(v)[0], O.pixel_norm(v))
    vv = v.clone().requires_grad_(True); dy = _seeded((5, 70), 10).double()
    (gx,) = torch.autograd.grad((O.pixel_norm(vv) * dy).sum(), vv)
    assert torch.allclose(SR.pixelnorm_bwd(dy, v)[0], gx)
    # blur_kxk with the [1,2,1] filter is the 3x3 blur; its S dominates |ref|
    t = np.outer([1, 2, 1], [1, 2, 1]).astype(np.float32).flatten() / 16
    r, S = SR.blur_kxk(x, t, 3, 1, 4, 4)
    assert torch.allclose(r, SR._blur121(x)) and bool((S >= r.abs()).all())
    # the parameter layouts of the 1x1 RGB convolutions
    w = torch.arange(12, dtype=torch.float64)
    assert SR.rgb_weight(w, 1, 3, 4).tolist() == [[0, 3, 6, 9], [1, 4, 7, 10], [2, 5, 8, 11]]
    assert SR.rgb_weight(w, 4, 1, 4).tolist() == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]]
    assert SR.colsum_chain(50, 16, torch.float32, False) == 1 and SR.colsum_chain(1 << 25, 16, torch.bfloat16, False) == 256
