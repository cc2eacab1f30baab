"""The version-1 UNet's GEMM-path convolutions, its head and its 16-bit image path, judged element by element.

The layers with Cin and Cout >= 64 run through launch_gemm in a form only the UNet's forward launches (kernels.h
gemm_params_unet_conv: a 3x3 convolution whose A operand may be a channel slice of the level's concat buffer);
dptx_op_unet_conv_gemm launches exactly that form.  Conventions of tests/test_gpu_gemm_elements.py: operands of
scaled_conv_operands (every pixel and every output channel a scale of its own), outputs that start as NaN with one guard row
behind row M, and every element inside gemm_elem_bound of the fp64 convolution of the 16-bit values actually stored.  A sliced
operand sits in a buffer x_pix_stride wide whose other channels are NaN.  tests/test_unet_bound_host.py shows on a CPU that the
bound's fp32 floor holds at the UNet's K (up to 13824) and what the head's bound rejects; profiles/unet_elements.md has the
worst |err| / bound of every case.  pytest -m gpu; the table check and the refusals need no GPU."""
import functools

import pytest
import torch

from omnidata_amd.engine import DTYPES, IO_DTYPES, load_library
from omnidata_amd.unet import unet_state_dict_spec
from tests.gpu_util import (TDT, UNET_HEAD_HW, UNET_HEAD_OC, assert_elements_inside, conv_ref64, debug_flags, f32_guards_intact,
                            gemm_elem_bound, guarded_f32, ptr, scaled_conv_operands, stream, unet_head_operands, unet_head_ref64)

gpu = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
MODES = ("bf16", "fp16")


def chan(i):
    return 16 << i


# ------------------------------------------------------------------------- a. every GEMM-path layer of the forward
# (layers, Cin, Cout, x_pix_stride, x_off, levels); level i = the input size / 2^i; c_i = chan(i)
UNET_GEMM_LAYERS = (
    [("down_blocks.1 conv2/3, up_blocks.2 conv2/3", 64, 64, 64, 0, (1, 2))] +
    [(f"down_blocks.{i} conv1", chan(i), chan(i + 1), 3 * chan(i), 2 * chan(i), (i,)) for i in range(2, 6)] +
    [(f"down_blocks.{i} conv2/3", chan(i + 1), chan(i + 1), chan(i + 1), 0, (i,)) for i in range(2, 6)] +
    [("mid_conv1..3", 1024, 1024, 1024, 0, (6,))] +
    [(f"up_blocks.{i} conv1", 3 * chan(i), chan(i), 3 * chan(i), 0, (i,)) for i in range(5, 1, -1)] +
    [(f"up_blocks.{i} conv2/3", chan(i), chan(i), chan(i), 0, (i,)) for i in range(5, 2, -1)])
# the distinct geometries (Cin, Cout, x_pix_stride, x_off, level)
UNET_GEMM_GEOMETRIES = sorted({(ci, co, xs, xo, lv) for _, ci, co, xs, xo, levels in UNET_GEMM_LAYERS for lv in levels},
                              key=lambda g: (g[4], g[0], g[1], g[3]))
# what unet.hip's small-channel kernel takes (unet_conv_small_supported), restated: (Cin, Cout) of a 3x3 layer; (3, 16) is the
# first layer behind the im2col
UNET_SMALL = {(3, 16), (16, 16), (16, 32), (32, 32), (32, 64), (48, 16), (96, 32)}
UNET_INPUTS = ((1, 64, 64), (3, 64, 128))   # (B, H, W) of the input image: the maps run from 32x32 down to 1x1 and 1x2


def test_table_covers_every_gemm_path_layer_of_the_model():
    """Every convolution of unet_state_dict_spec() is a 3x3 layer the small-channel kernel takes, the 1x1 of the head, or a row
    of the table above with its Cin, Cout, level and (for a down block's conv1: the skip slice of the concat buffer) slice."""
    assert len(UNET_GEMM_GEOMETRIES) == 18
    table = set(UNET_GEMM_GEOMETRIES)
    seen = set()
    for key, shape in unet_state_dict_spec(3).items():
        if len(shape) != 4:
            continue
        name = key[:-len(".weight")]
        cout, cin, k, _ = shape
        if name == "last_conv2":
            assert (k, cin) == (1, 16)                       # unet_gn_head_kernel
            continue
        assert k == 3, name
        if (cin, cout) in UNET_SMALL:
            continue
        parts = name.split(".")
        level = 6 if name.startswith("mid_conv") else int(parts[1]) if parts[0] in ("down_blocks", "up_blocks") else 0
        sliced = parts[0] == "down_blocks" and parts[-1] == "conv1"   # reads channels [2 c_i, 3 c_i) of CAT_i
        geo = (cin, cout, 3 * cin if sliced else cin, 2 * cin if sliced else 0, level)
        assert geo in table, (name, geo)
        seen.add(geo)
    assert seen == table, table - seen


def run_unet_conv(lib, mode, Xbuf, xs, xo, Wt, bias, B, H, W, Cin, Cout, flags=0):
    """-> the [M, Cout] output of one launch; the NaN guard row behind row M is checked"""
    M = B * H * W
    full = torch.full((M + 1, Cout), NAN, dtype=TDT[mode], device=DEV)
    with debug_flags(flags):
        rc = lib.dptx_op_unet_conv_gemm(DTYPES[mode], ptr(Xbuf), xs, xo, Xbuf.numel() * 2, ptr(Wt), ptr(bias), ptr(full), B, H, W,
                                        Cin, Cout, stream())
    assert rc == 0, (flags, rc)
    assert torch.isnan(full[M].float()).all(), "row M was written"
    return full[:M]


def unet_conv_case(mode, B, H, W, Cin, Cout, xs, xo, seed):
    """(X buffer [B, H, W, xs] with NaN outside the slice, Wt, bias, y, S): operands on the device, fp64 reference of the stored
    16-bit values"""
    X64, W64, b64, _ = scaled_conv_operands(B, H, W, Cin, Cout, 3, seed)
    tdt = TDT[mode]
    X = X64.to(tdt).to(DEV)
    Xbuf = torch.full((B, H, W, xs), NAN, dtype=tdt, device=DEV)
    Xbuf[..., xo:xo + Cin] = X
    Wt, bias = W64.to(tdt).to(DEV), b64.float().to(DEV)
    y, S = conv_ref64(X, Wt, bias, None, 1, 1, 1, H, W)
    return Xbuf, Wt, bias, y, S


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Bi,Hi,Wi", UNET_INPUTS)
@pytest.mark.parametrize("Cin,Cout,xs,xo,level", UNET_GEMM_GEOMETRIES)
def test_unet_gemm_layers_elements(mode, Bi, Hi, Wi, Cin, Cout, xs, xo, level):
    """dptx_op_unet_conv_gemm on each of the 18 GEMM-path geometries of the forward, at the maps of a 64x64 input with B = 1 and
    of a 64x128 input with B = 3: M from 1 (a 3x3 convolution on a 1x1 map: 8 of 9 taps are padding) to 6144, K up to 13824,
    the sliced A operand of every down block's conv1 on both kernels' offset arithmetic and on the tap-fastest k order."""
    lib = load_library()
    H, W = Hi >> level, Wi >> level
    Xbuf, Wt, bias, y, S = unet_conv_case(mode, Bi, H, W, Cin, Cout, xs, xo, seed=Cin + Cout + level)
    got = run_unet_conv(lib, mode, Xbuf, xs, xo, Wt, bias, Bi, H, W, Cin, Cout)
    assert_elements_inside(got.double().view(Bi, H, W, Cout), y, gemm_elem_bound(mode, y, S, 0),
                           f"unet conv {mode} {Cin}->{Cout} stride {xs} off {xo} level {level} B={Bi} {H}x{W}")


# ------------------------------------------------------------------------- b. the sliced operand on the larger tiles
# name -> (H, W, Cin, Cout, x_pix_stride, x_off, debug flags whose results must agree bit for bit); B = 1
UNET_SLICE_TILES = {
    # M = 33856: N % 128 == 0 and ceil(M / 128) = 265 >= 256 tiles: the 128x128 tile (4 waves); N = 128 rules the 256x256 tile out.
    # The forward launches this layer (down_blocks.2.conv1) at M = 36864 for 384x384 with B = 4
    "128x128": (184, 184, 64, 128, 192, 128, (0,)),
    # M = 28900: ceil(M / 128) = 226 < 256, N != 32, N >= 128 (no 256x64); 226 * (N / 64) = 452 >= 448: the 128x64 tile.
    # The forward: 320x320 with B = 5 (M = 32000: 250 * 2 = 500)
    "128x64": (170, 170, 64, 128, 192, 128, (0,)),
    # M = 52432: N % 256 == 0, K = 1152 >= 512, t256 = ceil(M / 256) = 205 >= 200, fill256 = 205 / 256 = 0.80 and
    # fill128 = 820 / 1024 = 0.80, 0.80 * 1.5 >= 0.80: gemm_pp_kernel, and with bias only its register-direct epilogue.  Flag 1:
    # the staged epilogue, flag 3: that and one block per tile.  The forward (down_blocks.3.conv1): 384x384 with B >= 23
    "256x256pp": (232, 226, 128, 256, 384, 256, (0, 1, 3)),
}


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tile", list(UNET_SLICE_TILES))
def test_unet_sliced_operand_on_the_larger_tiles(mode, tile):
    """The skip slice of the concat buffer (pixel stride 3 Cin, offset 2 Cin, NaN in the other channels) through the tiles the
    forward reaches at its larger sizes; the branch of launch_dt each case takes is derived in UNET_SLICE_TILES."""
    lib = load_library()
    H, W, Cin, Cout, xs, xo, flags = UNET_SLICE_TILES[tile]
    Xbuf, Wt, bias, y, S = unet_conv_case(mode, 1, H, W, Cin, Cout, xs, xo, seed=H + W)
    outs = [run_unet_conv(lib, mode, Xbuf, xs, xo, Wt, bias, 1, H, W, Cin, Cout, f).clone() for f in flags]
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), "debug flags 1 / 3 change the bits"
    assert_elements_inside(outs[0].double().view(1, H, W, Cout), y, gemm_elem_bound(mode, y, S, 0),
                           f"unet sliced conv {mode} {tile} {Cin}->{Cout} {H}x{W}")


def test_unet_conv_gemm_rejects_what_it_cannot_run(built_lib):
    """no launch happens: the plane dtypes, what launch_gemm refuses (Cin % 64, Cout % 32), a slice outside its pixel, a buffer
    smaller than the map"""
    lib = load_library()
    a = 1 << 20   # never dereferenced: every call is refused before a launch
    ok = dict(dtype=1, xs=64, xo=0, bytes=8 * 8 * 64 * 2, B=1, H=8, W=8, Cin=64, Cout=64)
    for change in (dict(dtype=2), dict(dtype=3), dict(dtype=5), dict(Cin=32, xs=32, bytes=8 * 8 * 32 * 2), dict(Cout=48),
                   dict(xs=72, xo=16, bytes=8 * 8 * 72 * 2), dict(xo=4, xs=72, bytes=8 * 8 * 72 * 2), dict(xs=68, bytes=8 * 8 * 68 * 2),
                   dict(bytes=8 * 8 * 64 * 2 - 2), dict(B=0), dict(H=0)):
        c = dict(ok, **change)
        rc = lib.dptx_op_unet_conv_gemm(c["dtype"], a, c["xs"], c["xo"], c["bytes"], a, a, a, c["B"], c["H"], c["W"], c["Cin"],
                                        c["Cout"], None)
        assert rc == -1, (change, rc)


# ------------------------------------------------------------------------- c. the head
@gpu
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("HW", UNET_HEAD_HW)
@pytest.mark.parametrize("OC", UNET_HEAD_OC)
def test_unet_head_elements(dtype, HW, OC):
    """dptx_op_unet_gn_head (last_bn + ReLU + last_conv2, fp32 NCHW out) on a caller-supplied (mean, rstd) table -- the fp64
    statistics of the stored input rounded to fp32 -- against fp64 of the same table, every element inside the derived bound of
    gpu_util.unet_head_ref64 (its docstring has the derivation; no measured constant).  B = 3, every (image, group) with
    statistics of its own; HW = 1, one short of and one past a block of 256 pixels, and 16 blocks.  The output lies between
    NaN guards."""
    lib = load_library()
    B, GUARD = 3, 512
    ops = unet_head_operands(dtype, B, HW, OC, seed=HW + OC)
    y, bound = unet_head_ref64(*ops)
    X, stats, gamma, beta, w, bias = (t.to(DEV).contiguous() for t in ops)
    buf, out = guarded_f32(B * OC * HW, GUARD)
    rc = lib.dptx_op_unet_gn_head(DTYPES[dtype], ptr(X), ptr(stats), ptr(gamma), ptr(beta), ptr(w), ptr(bias), ptr(out), B, HW, OC,
                                  stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert f32_guards_intact(buf, B * OC * HW, GUARD), "written outside the output"
    assert_elements_inside(out.view(B, OC, HW).double().cpu(), y, bound, f"unet head {dtype} HW={HW} OC={OC}")


def test_unet_head_rejects_bad_channel_counts(built_lib):
    lib = load_library()
    a = 1 << 20   # never dereferenced
    for dtype, OC, B, HW in ((1, 0, 1, 16), (1, 5, 1, 16), (0, -1, 1, 16), (2, 3, 1, 16), (1, 3, 0, 16), (1, 3, 1, 0)):
        assert lib.dptx_op_unet_gn_head(dtype, a, a, a, a, a, a, a, B, HW, OC, None) == -1, (dtype, OC, B, HW)


# ------------------------------------------------------------------------- d. the 16-bit image path of the first layer
@functools.lru_cache(maxsize=None)
def first_layer_weights(dtype):
    g = torch.Generator().manual_seed(41)
    Wp = torch.zeros(16, 32)
    Wp[:, :27] = torch.randn(16, 27, generator=g) * 27 ** -0.5
    return Wp.to(TDT[dtype]).to(DEV), (torch.randn(16, generator=g) * 0.2).to(DEV)


@gpu
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("io", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,W", [(2, 8, 32), (1, 13, 45)])
def test_first_layer_16bit_image_bitwise(dtype, io, B, H, W):
    """dptx_op_unet_conv3x3_io on a bf16 / fp16 image gives, bit for bit, the output and the GroupNorm records of DPTX_IO_FP32
    on image.float(): unet_im2col3_kernel reads the 16-bit elements directly.  One pixel in seven is an exact zero and the
    border pixels are the largest values, so a window that reads past the border instead of the zero padding changes bits.
    (An io outside the enum is refused.)"""
    lib = load_library()
    tio = {"bf16": torch.bfloat16, "fp16": torch.float16}[io]
    g = torch.Generator().manual_seed(B + H + W)
    img = torch.randn(B, 3, H, W, generator=g)
    img.view(-1)[::7] = 0.0
    img[:, :, 0, :], img[:, :, H - 1, :], img[:, :, :, 0], img[:, :, :, W - 1] = 5.0, -6.0, 7.0, -8.0
    img = img.to(tio).to(DEV).contiguous()
    Wp, bias = first_layer_weights(dtype)
    nrec = lib.dptx_op_unet_conv_records(H, W)
    res = []
    for x in (img, img.float().contiguous()):
        Y = torch.full((B, H, W, 16), NAN, dtype=TDT[dtype], device=DEV)
        part = torch.full((B, nrec, 8, 2), NAN, device=DEV)
        scratch = torch.full((B * H * W * 32,), NAN, dtype=TDT[dtype], device=DEV)
        rc = lib.dptx_op_unet_conv3x3_io(DTYPES[dtype], ptr(x), IO_DTYPES[x.dtype], ptr(Wp), ptr(bias), ptr(Y), ptr(part), B, H, W, 16,
                                         ptr(scratch), stream())
        assert rc == 0, rc
        res.append((Y, part, scratch))
    assert torch.isfinite(res[1][0].float()).all() and torch.isfinite(res[1][1]).all()
    for a, b in zip(*res):
        assert torch.equal(a.view(torch.int16 if a.dtype != torch.float32 else torch.int32),
                           b.view(torch.int16 if b.dtype != torch.float32 else torch.int32))
    assert lib.dptx_op_unet_conv3x3_io(DTYPES[dtype], ptr(img), 3, ptr(Wp), ptr(bias), ptr(res[0][0]), None, B, H, W, 16,
                                       ptr(res[0][2]), stream()) == -1
