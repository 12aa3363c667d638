"""The augmentation stage table (functional.AUG_STAGES): its rows against literals restated from include/sgx.h, what the parser and the
presets make of them, and the override hooks the Discriminator declares against the ones the table names.  No device needed."""
import itertools

import pytest

# (name, (draw hook, gate hook), ops in canonical order with their bits, mask, nu, ng, floats per table row, entry, takes H W, Function)
PIXEL = ("pixel", ("diffaug_override", "ada_gate_override"), {"color": 1, "xflip": 8, "rot90": 16, "translation": 2, "cutout": 4}, 31)
ROWS = [
    PIXEL + (None,) * 6,
    ("geom", ("geom_override", "geom_gate_override"), {"scale": 32, "rotate": 64, "aniso": 128}, 224,
     5, 3, 8, "sgx_ada_geom_matrix", False, "AdaGeomFn"),
    ("color", ("color_override", "color_gate_override"), {"brightness": 256, "contrast": 512, "lumaflip": 1024, "hue": 2048, "saturation": 4096},
     7936, 8, 5, 12, "sgx_ada_color_matrix", False, "AdaColorFn"),
    ("filter", ("filter_override", "filter_gate_override"), {"imgfilter": 8192}, 8192, 8, 4, 22, "sgx_ada_filter_matrix", False, "AdaFilterFn"),
    ("corrupt", ("corrupt_override", "corrupt_gate_override"), {"noise": 16384, "imgcutout": 32768}, 49152,
     6, 2, 8, "sgx_ada_corrupt_table", True, "AdaCorruptFn"),
]
ORDER = ("color", "xflip", "rot90", "translation", "cutout", "scale", "rotate", "aniso", "brightness", "contrast", "lumaflip", "hue",
         "saturation", "imgfilter", "noise", "imgcutout")
FULL = ",".join(ORDER)
HOOKS = {"diffaug_override", "ada_gate_override", "geom_override", "geom_gate_override", "color_override", "color_gate_override",
         "filter_override", "filter_gate_override", "corrupt_override", "corrupt_gate_override"}


def test_rows_are_the_headers_facts():
    from stylegan.pytorch_amd import functional as F
    assert [tuple(s) for s in F.AUG_STAGES] == ROWS
    for s, row in zip(F.AUG_STAGES, ROWS):
        assert tuple(s.bits) == tuple(row[2])                               # dict equality ignores the order; the canonical order counts
        assert isinstance(getattr(F, s.fn), type) if s.fn else s.name == "pixel"
    assert [s.mask for s in F.AUG_STAGES] == [31, 224, 7936, 8192, 49152]
    bits = [b for s in F.AUG_STAGES for b in s.bits.values()]
    assert all(a & b == 0 for a, b in itertools.combinations(bits, 2)) and all(b > 0 for b in bits)
    assert all(s.mask == sum(s.bits.values()) for s in F.AUG_STAGES)


def test_parser_order_is_the_rows_ops_concatenated():
    from stylegan.pytorch_amd import functional as F
    assert sum((tuple(s.bits) for s in F.AUG_STAGES), ()) == ORDER
    assert F.diffaug_policy_bits(FULL) == 65535
    for s in F.AUG_STAGES:
        assert F.diffaug_policy_bits(",".join(s.bits)) == s.mask
        for op, bit in s.bits.items():
            assert F.diffaug_policy_bits(op) == bit
    with pytest.raises(ValueError, match=f"in the order {FULL}"):
        F.diffaug_policy_bits("scale,color")
    with pytest.raises(ValueError, match=rf"unknown DiffAugment op 'blur' in 'blur' \(known: {FULL}\)"):
        F.diffaug_policy_bits("blur")
    assert F.diffaug_policy_bits(F.ada_preset("bgcfnc")) == 65530


def test_derived_constants_keep_their_values():
    from stylegan.pytorch_amd import functional as F
    assert (F.DIFFAUG_OPS, F.DIFFAUG_BITS, F.DIFFAUG_PIXEL_MASK, F.DIFFAUG_BLIT_BITS) == (tuple(PIXEL[2]), PIXEL[2], 31, 24)
    for row in ROWS[1:]:
        up = row[0].upper()
        assert (getattr(F, f"DIFFAUG_{up}_OPS"), getattr(F, f"DIFFAUG_{up}_BITS"), getattr(F, f"DIFFAUG_{up}_MASK")) == \
            (tuple(row[2]), row[2], row[3])


def test_every_declared_hook_is_in_the_table():
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd.GAN import Discriminator
    declared = {k for k in vars(Discriminator) if k.endswith("_override")}
    assert declared == {h for s in F.AUG_STAGES for h in s.hooks} == HOOKS
