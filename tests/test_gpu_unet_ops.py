"""Op-level checks of the version-1 UNet kernels (omnidata_amd/csrc/unet.hip, include/dptx.h dptx_op_unet_*) against fp64
references of the same 16-bit operands.  pytest -m gpu."""
import pytest
import torch
import torch.nn.functional as F

from omnidata_amd.engine import DTYPES, load_library
from tests.gpu_util import OUT_TOL, TDT, group_max, nhwc_with_group_stats, per_group_err, ptr, stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U32 = 2.0 ** -24                                 # fp32 unit roundoff
STEP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}   # unit roundoff of the 16-bit types (round to nearest)


def rnd(*shape, dtype, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(TDT[dtype]).to(DEV)


# ------------------------------------------------------------------------------------------------ small-channel 3x3 convolution
CONV_CH = [(3, 16), (16, 16), (16, 32), (32, 32), (32, 64), (48, 16), (96, 32)]
# (2, 5, 7), (1, 13, 45), (3, 16, 16): partial 8 x 32 tiles in both directions -- 13 rows: the second tile row has 5 live rows, so
# wave 2 stores one of its two rows and wave 3 none; 45 and 16 columns: 13 / 16 live lanes; 5 x 7: one tile, most of it outside
CONV_SHAPES = [(3, 32, 32), (2, 64, 64), (1, 64, 128), (2, 5, 7), (1, 13, 45), (3, 16, 16)]
# the slices the forward itself reads on this kernel: (Cin, Cout, pixel stride, offset) -- the skip slices of CAT_0 and CAT_1
FORWARD_SLICES = [(16, 32, 48, 32), (32, 64, 96, 64)]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,W", CONV_SHAPES)
@pytest.mark.parametrize("Cin,Cout", CONV_CH)
def test_small_channel_conv(dtype, B, H, W, Cin, Cout):
    """dptx_op_unet_conv3x3 against a float64 conv2d of the same 16-bit operands, element by element.

    Bound per element, with S = sum |a||w| + |bias| over the K = 9 Cin products of that output (an fp64 convolution of the
    absolute values): the MFMA accumulates K products (exact in fp32: 8 / 11-bit significands) and the bias in some order in
    fp32, so |acc - exact| <= K u32 S (the worst-case bound of a length-K sum); the store rounds once: STEP (|exact| + K u32 S).

    Every image's top row is +200 and its bottom row -200 in every channel: a halo that reads the neighbouring image's row
    instead of zero moves the outputs next to the border by hundreds.  (48, 16) and (96, 32) read a channel slice of a wider
    buffer (pixel stride Cin + 24, offset 8) whose other channels are NaN.

    The GroupNorm(8) records of the epilogue, summed over the tiles, against the fp64 (sum, sum of squares) of the exact
    outputs per (image, group): every element may be off by its bound e above (sum: sum e; squares: sum 2 |v| e + e^2), and a
    record is built by at most 64 fp32 additions (2 per lane, 5 butterfly steps, 4 waves x up to 4 channel pairs) before the
    records are added in double: 64 u32 sum |v| (resp. sum v^2)."""
    small_channel_conv(dtype, B, H, W, Cin, Cout)


def small_channel_conv(dtype, B, H, W, Cin, Cout, x_slice=None, records=True):
    """One launch of dptx_op_unet_conv3x3 and the checks of test_small_channel_conv's docstring -> Y.  x_slice = (pixel stride,
    offset) of the input's channel slice (default: the test's own rule); records = False: gn_part = NULL, no record checks."""
    lib = load_library()
    tdt = TDT[dtype]
    seed = 100 * Cin + Cout
    Wt = rnd(Cout, Cin, 3, 3, dtype=dtype, scale=(9 * Cin) ** -0.5, seed=seed)                # OIHW
    bias = (torch.randn(Cout, generator=torch.Generator().manual_seed(seed + 1)) * 0.2).to(DEV)
    x = rnd(B, Cin, H, W, dtype=dtype, seed=seed + 2)                                         # NCHW, 16-bit values
    x[:, :, 0, :] = 200.0
    x[:, :, H - 1, :] = -200.0
    Y = torch.full((B, H, W, Cout), float("nan"), dtype=tdt, device=DEV)
    nrec = lib.dptx_op_unet_conv_records(H, W)
    assert nrec == ((H + 7) // 8) * ((W + 31) // 32)
    part = torch.full((B, nrec, 8, 2), float("nan"), device=DEV) if records else None
    if Cin == 3:
        Xdev = x.float().contiguous()                                                         # the caller's fp32 NCHW image
        Wp = torch.zeros(Cout, 32, dtype=tdt, device=DEV)
        Wp[:, :27] = Wt.permute(0, 2, 3, 1).reshape(Cout, 27)
        scratch = torch.empty(B * H * W * 32, dtype=tdt, device=DEV)
        rc = lib.dptx_op_unet_conv3x3(DTYPES[dtype], ptr(Xdev), 0, 0, ptr(Wp), ptr(bias), ptr(Y), ptr(part), B, H, W, 3, Cout,
                                      ptr(scratch), stream())
    else:
        Wp = Wt.permute(0, 2, 3, 1).contiguous()                                              # [O][ky][kx][I]
        if x_slice is not None or Cin in (48, 96):
            stride, off = x_slice if x_slice is not None else (Cin + 24, 8)
            Xdev = torch.full((B, H, W, stride), float("nan"), dtype=tdt, device=DEV)
            Xdev[..., off:off + Cin] = x.permute(0, 2, 3, 1)
        else:
            stride, off = Cin, 0
            Xdev = x.permute(0, 2, 3, 1).contiguous()
        rc = lib.dptx_op_unet_conv3x3(DTYPES[dtype], ptr(Xdev), stride, off, ptr(Wp), ptr(bias), ptr(Y), ptr(part), B, H, W, Cin,
                                      Cout, None, stream())
    assert rc == 0, rc
    ref = F.conv2d(x.double(), Wt.double(), bias.double(), padding=1)                         # [B, Cout, H, W]
    S = F.conv2d(x.double().abs(), Wt.double().abs(), bias.double().abs(), padding=1)
    K = 9 * Cin
    e_acc = K * U32 * S
    bound = e_acc + STEP[dtype] * (ref.abs() + e_acc) + 2.0 ** -40
    got = Y.double().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    ratio = ((got - ref).abs() / bound).max()
    print(f"\n[unet conv {dtype} {Cin}->{Cout} B={B} {H}x{W}] worst |err| / bound {float(ratio):.3f}")
    assert ratio <= 1.0
    if not records:
        return Y
    # records
    cpg = Cout // 8
    rs = part.double().sum(1)                                                                  # [B, 8, 2]
    v = ref.reshape(B, 8, cpg * H * W)
    eb = bound.reshape(B, 8, cpg * H * W)
    b1 = eb.sum(-1) + 64 * U32 * v.abs().sum(-1)
    b2 = (2 * v.abs() * eb + eb * eb).sum(-1) + 64 * U32 * (v * v).sum(-1)
    r1 = ((rs[..., 0] - v.sum(-1)).abs() / b1).max()
    r2 = ((rs[..., 1] - (v * v).sum(-1)).abs() / b2).max()
    print(f"  records: sum {float(r1):.3f}, squares {float(r2):.3f} of their bounds")
    assert r1 <= 1.0 and r2 <= 1.0
    return Y


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,W", [(3, 32, 32), (1, 13, 45)])
@pytest.mark.parametrize("Cin,Cout,stride,off", FORWARD_SLICES)
def test_small_channel_conv_forward_slices(dtype, B, H, W, Cin, Cout, stride, off):
    """test_small_channel_conv on the slices the forward reads: 16 -> 32 from channels [32, 48) of a 48-wide buffer (down_blocks.0
    conv1) and 32 -> 64 from [64, 96) of a 96-wide one (down_blocks.1 conv1); the other channels are NaN."""
    small_channel_conv(dtype, B, H, W, Cin, Cout, x_slice=(stride, off))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("Cin,Cout", CONV_CH)
def test_small_channel_conv_without_records(dtype, Cin, Cout):
    """gn_part = NULL (the kernel returns before the record reduction): Y is inside its bound and equals, bit for bit, the Y of
    the run that writes records, on a map with partial tiles."""
    B, H, W = 2, 13, 45
    with_rec = small_channel_conv(dtype, B, H, W, Cin, Cout)
    without = small_channel_conv(dtype, B, H, W, Cin, Cout, records=False)
    assert torch.equal(with_rec.view(torch.int16), without.view(torch.int16))


def test_small_channel_conv_rejects_what_it_cannot_run():
    lib = load_library()
    t = torch.zeros(4096, dtype=torch.float16, device=DEV)
    f = torch.zeros(64, device=DEV)
    for Cin, Cout, stride, off in ((64, 64, 64, 0), (16, 48, 16, 0), (16, 16, 20, 0), (16, 16, 24, 4), (16, 16, 16, 8)):
        assert lib.dptx_op_unet_conv3x3(1, ptr(t), stride, off, ptr(t), ptr(f), ptr(t), None, 1, 8, 8, Cin, Cout, None, stream()) == -1
    assert lib.dptx_op_unet_conv3x3(2, ptr(t), 16, 0, ptr(t), ptr(f), ptr(t), None, 1, 8, 8, 16, 16, None, stream()) == -1   # a plane dtype
    assert lib.dptx_op_unet_conv3x3(1, ptr(t), 0, 0, ptr(t), ptr(f), ptr(t), None, 1, 8, 8, 3, 16, None, stream()) == -1     # no scratch


# ------------------------------------------------------------------------------------------------ GroupNorm(8) + ReLU
def gn8_ref(X, g, b):
    """fp64 GroupNorm(8) of the stored NHWC [B,H,W,C] input, before the ReLU"""
    return F.group_norm(X.double().permute(0, 3, 1, 2), 8, g.double(), b.double(), 1e-5).permute(0, 2, 3, 1)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("form", ["dense", "slice", "pool", "pool-only"])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 2), (64, 64)])
@pytest.mark.parametrize("C", [16, 64, 1024])
def test_groupnorm8_relu(dtype, form, H, W, C):
    """dptx_op_unet_groupnorm on inputs whose every (image, group) has statistics of its own, against fp64 group_norm, judged
    per (image, group) relative to that group's max |gn(x)| before the ReLU.

    Bar: the output rounding (OUT_TOL) plus the error of the fp32 statistics.  The sums of x and x^2 are built by at most k = 64
    fp32 additions per record (16 per thread, then the block's fixed-order sum) and combined in double, so the variance is off
    by 2 k u32 E[x^2] at most and rstd by q k u32 relatively, q = E[x^2] / (var + eps); the mean by k u32 sqrt(E[x^2]), which
    moves the output by sqrt(q) k u32 |gamma|.  q is 3.25 for these inputs, except in groups of a few elements (HW = 1) that
    happen to be almost constant, where it is large and says so.

    form 'slice': the result goes into channels [8, 8 + C) of a buffer C + 24 wide filled with a poison value that must survive;
    'pool': additionally the 2x2 / 2 max-pooled result into a slice of its own (odd sizes must be refused);
    'pool-only': Y = NULL and P only, what every down block's bn3 launches -- once into a slice (pixel stride 3 C, offset 2 C:
    the skip slice of the next level's concat buffer) and once dense (the last down block) -- must give, bit for bit, the pooled
    values of the 'pool' form on the same input (which the 'pool' case judges against fp64); the rest of the slice stays."""
    lib = load_library()
    B, tdt = 3, TDT[dtype]
    X = nhwc_with_group_stats(B, H * W, C, groups=8, seed=70 + C + H).to(tdt).to(DEV).reshape(B, H, W, C)
    gen = torch.Generator().manual_seed(C + W)
    g = (0.5 + torch.rand(C, generator=gen)).to(DEV)
    b = (0.6 * torch.rand(C, generator=gen) - 0.3).to(DEV)
    POISON = 7.0
    ys, yo = (C, 0) if form == "dense" else (C + 24, 8)
    Y = torch.full((B, H, W, ys), POISON, dtype=tdt, device=DEV)
    P = torch.full((B, max(H // 2, 1), max(W // 2, 1), C + 16), POISON, dtype=tdt, device=DEV) if form in ("pool", "pool-only") else None
    nrec = lib.dptx_op_unet_gn_records(H * W, C)
    assert nrec >= 1
    scratch = torch.empty(B * (nrec * 16 + 16), device=DEV)
    rc = lib.dptx_op_unet_groupnorm(DTYPES[dtype], ptr(X), ptr(g), ptr(b), ptr(Y), ys, yo, ptr(P), C + 16, 16, B, H, W, C, 1e-5,
                                    ptr(scratch), stream())
    if form in ("pool", "pool-only") and (H % 2 or W % 2):
        assert rc == -1
        if form == "pool-only":
            assert lib.dptx_op_unet_groupnorm(DTYPES[dtype], ptr(X), ptr(g), ptr(b), None, 0, 0, ptr(P), C + 16, 16, B, H, W, C, 1e-5,
                                              ptr(scratch), stream()) == -1
        return
    assert rc == 0, rc
    if form == "pool-only":
        for ps, po in ((3 * C, 2 * C), (C, 0)):
            P1 = torch.full((B, H // 2, W // 2, ps), POISON, dtype=tdt, device=DEV)
            scratch.fill_(float("nan"))
            assert lib.dptx_op_unet_groupnorm(DTYPES[dtype], ptr(X), ptr(g), ptr(b), None, 0, 0, ptr(P1), ps, po, B, H, W, C, 1e-5,
                                              ptr(scratch), stream()) == 0
            assert torch.equal(P1[..., po:po + C].contiguous().view(torch.int16), P[..., 16:].contiguous().view(torch.int16)), (ps, po)
            assert (P1[..., :po] == POISON).all()
        return
    pre = gn8_ref(X, g, b)
    ref = F.relu(pre)
    xg = X.double().reshape(B, H * W, 8, C // 8).transpose(1, 2).reshape(B, 8, -1)
    q = (xg * xg).mean(-1) / (xg.var(-1, unbiased=False) + 1e-5)
    scale = group_max(pre, 8)
    bar = OUT_TOL[dtype] + 64 * U32 * (q + q.sqrt() * float(g.max()) / scale)
    err = per_group_err(Y[..., yo:yo + C], ref, groups=8, scale=scale)
    print(f"\n[unet gn {dtype} {form} {H}x{W} C={C}] worst (image, group) err / bar {float((err / bar).max()):.3f}, max q {float(q.max()):.1f}")
    assert (err <= bar).all(), torch.nonzero(err > bar)[:5].tolist()
    if form != "dense":
        assert (Y[..., :yo] == POISON).all() and (Y[..., yo + C:] == POISON).all()
    if form == "pool":
        pref = F.max_pool2d(ref.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
        perr = per_group_err(P[..., 16:], pref, groups=8, scale=scale)
        assert (perr <= bar).all()
        assert (P[..., :16] == POISON).all()
        # the pooled copy is the maximum of the stored full-size values, bit for bit
        assert torch.equal(P[..., 16:], F.max_pool2d(Y[..., yo:yo + C].float().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).to(tdt))


# ------------------------------------------------------------------------------------------------ bilinear x2, align_corners=False
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 2), (24, 40)])
def test_upsample2x_half_pixel(dtype, H, W):
    """dptx_op_unet_upsample2x into a channel slice against F.interpolate(scale_factor=2, bilinear, align_corners=False) in fp64:
    the stored value must be the storage type's rounding of the fp32 result, to the last bit; the poison around the slice stays."""
    upsample2x_half_pixel(dtype, 2, H, W, 24, 24 + 16, 8)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("H,W,C,ys", [(1, 1, 1024, 1536), (2, 4, 512, 768)])
def test_upsample2x_forward_extremes(dtype, H, W, C, ys):
    """The forward's extremes, same check: the 1x1 map of 1024 channels into channels [0, 1024) of the 1536-wide concat buffer
    of level 5, and 2x4 of 512 into [0, 512) of 768 (level 4 of a 64x128 input); the skip slice behind them is poison and stays."""
    upsample2x_half_pixel(dtype, 2, H, W, C, ys, 0)


def upsample2x_half_pixel(dtype, B, H, W, C, ys, yo):
    lib = load_library()
    tdt = TDT[dtype]
    X = rnd(B, H, W, C, dtype=dtype, seed=90 + H)
    Y = torch.full((B, 2 * H, 2 * W, ys), 7.0, dtype=tdt, device=DEV)
    assert lib.dptx_op_unet_upsample2x(DTYPES[dtype], ptr(X), ptr(Y), B, H, W, C, ys, yo, stream()) == 0
    ref = F.interpolate(X.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    want = ref.float().to(tdt)
    got = Y[..., yo:yo + C]
    assert torch.equal(got.view(torch.int16), want.contiguous().view(torch.int16)), float((got.double() - ref).abs().max())
    assert (Y[..., :yo] == 7.0).all() and (Y[..., yo + C:] == 7.0).all()
