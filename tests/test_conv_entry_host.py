"""CPU: srcgan_conv_igemm refuses a malformed descriptor with the documented message, before any HIP call.

The entry (csrc/conv_entry.hip) checks the descriptor, builds the kernels' parameter block and routes to a kernel family; every
refusal -- the entry's own and the routes' -- comes before the first call into the HIP runtime, so the library can be asked on a
machine without a GPU.  The pointers are fake 16-byte-aligned integers and are never dereferenced.  The expected texts were recorded
from the library as it was before the entry got a file of its own; they are part of the C ABI's behaviour (callers and
tests/test_gpu_fullsize.py match on them)."""
import ctypes as C

import pytest

X, WP, Y, AUX = 0x10000, 0x20000, 0x30000, 0x40000

# a well-formed bf16 3x3 stride-1 convolution, 32 -> 32 channels on 8x8 pixels; every case changes a few fields of it
BASE = dict(x=X, wp=WP, y=Y, dtype=1, kh=3, kw=3, stride=1, B=1, H=8, W=8, Cin=32, x_cs=32, OH=8, OW=8, Cout=32, YH=8, YW=8, y_cs=32,
            pad_y=1, pad_x=1, os=1, alpha=1.0)
SIGN_RULE = ("srcgan_conv_igemm: sign masks need a 3x3 s1 16-bit conv with Cout == 32 on a blocked input, unscaled output (act for sign_out, "
             "no mz beside sign_in); or Cout == 64: sign_out of the 1x1 four-parity form with act, sign_in of a 3x3 s1 conv without other operands")
UP = dict(kh=1, kw=1, pad_y=0, pad_x=0, os=2, YH=16, YW=16, npar=4, wpar_stride=4096)          # the 1x1 four-parity form, well-formed

# a single image of 8185 x 4100 pixels with 64 bf16 channels: 4,295,488,000 bytes
BIG = dict(H=8185, W=4100, Cin=64, x_cs=64, OH=8185, OW=4100, YH=8185, YW=4100)
IMAGE_RULE = ("srcgan_conv_igemm: one image of the input must be below 2 GiB for this kernel (%d x %d pixels of %d bytes); only the loader-specialised "
              "3x3 stride-1 form (pad 1, whole 64-byte input chunks, 18 rows below 2 GiB) takes larger images")

CASES = [
    ("null_pointer", dict(y=None), "srcgan_conv_igemm: null pointer"),
    ("bad_dtype", dict(dtype=7), "srcgan_conv_igemm: bad dtype 7"),
    ("non_positive_dimension", dict(H=0), "srcgan_conv_igemm: non-positive dimension"),
    ("channels_not_in_pieces", dict(Cin=12), "srcgan_conv_igemm: input channels/stride/offset (12,32,0) must be multiples of 8"),
    ("channels_not_in_pieces_f32", dict(dtype=0, x_coff=2, Cin=4), "srcgan_conv_igemm: input channels/stride/offset (4,32,2) must be multiples of 4"),
    ("slice_beyond_stride", dict(y_coff=8), "srcgan_conv_igemm: channel slice exceeds stride"),
    ("blocked_input_not_3x3", dict(kh=1, kw=1, x_plane=4096), "srcgan_conv_igemm: a blocked-layout input is supported by the 3x3 stride-1 kernel only"),
    ("misaligned_pointer", dict(x=X + 8), "srcgan_conv_igemm: x/wp must be 16-byte aligned"),
    ("bad_output_offset", dict(os=2, oa=2, YH=32, YW=32), "srcgan_conv_igemm: bad output scale/offset"),
    ("output_beyond_tensor", dict(OH=9), "srcgan_conv_igemm: output extent exceeds tensor"),
    ("sign_mask_rule", dict(dtype=0, sign_out=AUX, act=1, x_plane=4096), SIGN_RULE),
    ("npar_3x3_rule", dict(npar=4, wpar_stride=4096),
     "srcgan_conv_igemm: npar == 4 with a 3x3 kernel is the transposed stride-2 form: stride 2, pad 1, os 2, oa == ob == 0, OH x OW = H x W, "
     "YH x YW = 2H x 2W, the four parity packs wpar_stride bytes apart, interleaved tensors, no sign masks"),
    ("npar_1x1_rule", dict(UP, os=1, YH=8, YW=8),
     "srcgan_conv_igemm: npar == 4 with a 1x1 kernel needs os == 2, oa == ob == 0 and the four packs wpar_stride bytes apart"),
    ("npar_1x1_sign_out_needs_16_bytes", dict(UP, Cout=64, y_cs=64, act=1, sign_out=AUX, y=Y + 8),
     "srcgan_conv_igemm: sign_out of the 1x1 four-parity form needs 16-byte accessible output channels"),
    ("npar_other_rule", dict(kh=2, kw=2, npar=2, wpar_stride=4096),
     "srcgan_conv_igemm: npar must be 0 or 4 (2x2 stride-1 parity packs wpar_stride bytes apart, interleaved tensors, no bias / sign masks)"),
    ("npar_2x2_needs_16_bytes", dict(kh=2, kw=2, npar=4, wpar_stride=4096, os=2, YH=16, YW=16, Cout=4, y_cs=4),
     "srcgan_conv_igemm: npar == 4 needs output / mask channels, strides and offsets that are multiples of 16 bytes (and channel planes below 2 GiB)"),
    ("deconv_k3s2_needs_16_bytes", dict(stride=2, npar=4, wpar_stride=4096, os=2, YH=16, YW=16, Cout=4, y_cs=4),
     "srcgan_conv_igemm: the transposed 3x3 stride-2 form needs output channels, strides and offsets that are multiples of 16 bytes"),
    ("sign_mask_needs_loader_kernel", dict(sign_in=AUX, x_plane=4096, pad_y=0, pad_x=0),
     "conv3x3: sign masks are only handled by the loader-specialised 16-bit kernel (Cout == 32, or Cout == 64 read-only without other operands)"),
    # one image of 2 GiB or more: every kernel family but the loader-specialised 3x3 stride-1 one carries 32-bit offsets inside an image
    ("image_2gib_generic", dict(BIG, kh=2, kw=2, stride=2, pad_y=0, pad_x=0, OH=4092, OW=2050, YH=4092, YW=2050), IMAGE_RULE % (8185, 4100, 128)),
    ("image_2gib_1x1_pair", dict(BIG, **dict(UP, YH=16370, YW=8200)), IMAGE_RULE % (8185, 4100, 128)),
    ("image_2gib_par4", dict(BIG, kh=2, kw=2, npar=4, wpar_stride=4096, os=2, YH=16370, YW=8200), IMAGE_RULE % (8185, 4100, 128)),
    ("image_2gib_deconv", dict(BIG, stride=2, npar=4, wpar_stride=4096, os=2, YH=16370, YW=8200), IMAGE_RULE % (8185, 4100, 128)),
    ("image_2gib_3x3_pad0", dict(BIG, pad_y=0, pad_x=0, OH=8183, OW=4098), IMAGE_RULE % (8185, 4100, 128)),
    ("image_2gib_3x3_wide_rows", dict(BIG, H=18, W=310700, Cin=192, x_cs=192, OH=18, OW=310700, YH=18, YW=310700), IMAGE_RULE % (18, 310700, 384)),
    ("unsupported_kernel", dict(kh=6, kw=6, pad_y=2, pad_x=2), "srcgan_conv_igemm: unsupported kernel 6x6 stride 1"),
]


@pytest.fixture(scope="module")
def lib():
    from srcgan_amd import build, _native
    build.build(verbose=False)
    return _native.lib()


@pytest.mark.parametrize("name,change,message", CASES, ids=[c[0] for c in CASES])
def test_malformed_descriptor_is_refused_with_its_message(lib, name, change, message):
    from srcgan_amd import _native as N
    d = N.ConvDesc(**dict(BASE, **change))
    assert lib.srcgan_conv_igemm(C.byref(d), None) == 1
    assert lib.srcgan_last_error().decode() == message


def test_case_table_covers_every_refusal_of_the_entry():
    """one case per SG_REQUIRE of the entry's check and route steps: a new rule needs a case here"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "srcgan_amd", "csrc", "conv_entry.hip")).read()
    rules = re.findall(r'SG_REQUIRE\(.*?"(srcgan_conv_igemm: [^"%]*)', src, flags=re.S)
    assert len(rules) >= 14
    for r in rules:
        assert any(m.startswith(r) for _, _, m in CASES), r
