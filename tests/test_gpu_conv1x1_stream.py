"""The streaming 1x1 kernel (csrc/conv1x1.hip) against the tiled kernels it replaces (dptx_debug_set_gemm_flags 8: never take
it), against fp32, and against itself at another batch size.  Flag 0 is the dispatch of the forward, which takes the kernel
only in the (K, N, stride) classes where it measured faster; flag 16 takes it for every launch it can serve, so that the
classes left on the tiled kernels (K = 256 with N = 1024, stride 2, the small out_conv maps) keep their coverage too: every
comparison below runs with both.  Shapes: the smallest at which it can go wrong -- 96 rows per image (three GroupNorm records; M = 288: a block's four 32-row waves straddle image boundaries and the last block is ragged),
M = 32 (one wave of one block has work), stride 2, and every (K, N) class the dispatch knows (K = 64 / 128 / 256; one, two
and eight W panels; cpg 2 .. 32)."""
import pytest
import torch
import torch.nn.functional as F

from omnidata_amd.engine import DTYPES, load_library
from tests.gpu_util import OUT_TOL, TDT, ptr, rel_err, stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# B, H, W, Cin, Cout, stride, records (GroupNorm op) or bias + ReLU (plain conv op)
GN_CASES = [(3, 8, 12, 64, 256, 1), (3, 8, 12, 64, 64, 1), (3, 8, 12, 256, 64, 1), (3, 8, 12, 128, 512, 1),
            (3, 8, 12, 256, 1024, 1), (1, 4, 8, 64, 256, 1), (1, 4, 8, 256, 1024, 1), (3, 16, 16, 256, 512, 2)]
PLAIN_CASES = [(3, 8, 12, 256, 256, 1), (1, 4, 8, 256, 256, 1)]
_cache = {}


def rnd(*shape, dtype, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(TDT[dtype]).to(DEV)


def operands(dtype, case):
    B, H, W, Cin, Cout, stride = case
    key = ("ops", dtype, case)
    if key not in _cache:
        g = torch.Generator(device="cpu").manual_seed(33)
        _cache[key] = (rnd(B, H, W, Cin, dtype=dtype, seed=30), rnd(Cout, 1, 1, Cin, dtype=dtype, scale=Cin ** -0.5, seed=31),
                       torch.randn(Cout, generator=g).to(DEV), torch.randn(Cout, generator=g).to(DEV))
    return _cache[key]


def run_gn(dtype, case, flags, image=None):
    """(raw conv output, normalised + ReLU'd output, records [B, blocks, 32, 2]) of dptx_op_conv_groupnorm; image: that one alone"""
    key = ("gn", dtype, case, flags, image)
    if key in _cache:
        return _cache[key]
    lib = load_library()
    B, H, W, Cin, Cout, stride = case
    X, Wt, g, b = operands(dtype, case)
    if image is not None:
        X, B = X[image:image + 1].contiguous(), 1
    Ho, Wo = H // stride, W // stride
    Yraw = torch.empty(B, Ho, Wo, Cout, device=DEV, dtype=TDT[dtype])
    Y = torch.empty_like(Yraw)
    rec = torch.full((B, Ho * Wo // 32, 32, 2), float("nan"), device=DEV)
    try:
        assert lib.dptx_debug_set_gemm_flags(flags) == 0
        rc = lib.dptx_op_conv_groupnorm(DTYPES[dtype], ptr(X), ptr(Wt), ptr(Yraw), ptr(g), ptr(b), None, ptr(Y), B, H, W, Cin, Cout,
                                        1, stride, 0, 0, Ho, Wo, 1, 1e-5, ptr(rec), stream())
    finally:
        lib.dptx_debug_set_gemm_flags(0)
    assert rc == 0
    torch.cuda.synchronize()
    _cache[key] = (Yraw, Y, rec)
    return _cache[key]


def run_plain(dtype, case, flags, image=None):
    """conv + bias + ReLU (refinenet out_conv's epilogue with the activation switched on as well), no records"""
    key = ("plain", dtype, case, flags, image)
    if key in _cache:
        return _cache[key]
    lib = load_library()
    B, H, W, Cin, Cout, stride = case
    X, Wt, bias, _ = operands(dtype, case)
    if image is not None:
        X, B = X[image:image + 1].contiguous(), 1
    Y = torch.empty(B, H // stride, W // stride, Cout, device=DEV, dtype=TDT[dtype])
    try:
        assert lib.dptx_debug_set_gemm_flags(flags) == 0
        rc = lib.dptx_op_conv(DTYPES[dtype], ptr(X), ptr(Wt), ptr(bias), None, ptr(Y), B, H, W, Cin, Cout, 1, stride, 0, 0,
                              H // stride, W // stride, 0, 1, stream())
    finally:
        lib.dptx_debug_set_gemm_flags(0)
    assert rc == 0
    torch.cuda.synchronize()
    _cache[key] = Y
    return Y


def conv32(X, Wt, bias, stride):
    """fp32 convolution of the 16-bit operands, NHWC"""
    y = F.conv2d(X.float().permute(0, 3, 1, 2), Wt.float().permute(0, 3, 1, 2), bias, stride)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", GN_CASES)
def test_stream_records_and_outputs_equal_tiled_bitwise(dtype, case):
    old = run_gn(dtype, case, 8)
    for flags in (0, 16):
        new = run_gn(dtype, case, flags)
        assert torch.equal(new[0], old[0]), flags        # raw convolution output
        assert torch.equal(new[2], old[2]), flags        # GroupNorm records (every record written: no NaN left)
        assert not torch.isnan(new[2]).any(), flags
        assert torch.equal(new[1], old[1]), flags        # normalised output


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", PLAIN_CASES)
def test_stream_bias_relu_equals_tiled_bitwise(dtype, case):
    assert torch.equal(run_plain(dtype, case, 0), run_plain(dtype, case, 8))
    assert torch.equal(run_plain(dtype, case, 16), run_plain(dtype, case, 8))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", GN_CASES)
def test_stream_conv_groupnorm_against_fp32(dtype, case):
    """The bound and the form of tests/test_gpu_ops.py::test_conv_groupnorm_fused_stats: raw output against the fp32 convolution,
    the normalised output against group_norm's fp32 statistics of that convolution applied to the stored map."""
    B, H, W, Cin, Cout, stride = case
    X, Wt, g, b = operands(dtype, case)
    Yraw, Y, rec = run_gn(dtype, case, 16)
    raw = conv32(X, Wt, None, stride)
    assert rel_err(Yraw.float(), raw) < OUT_TOL[dtype]
    xr = raw.permute(0, 3, 1, 2).reshape(B, 32, -1)
    mean, var = xr.mean(-1), xr.var(-1, unbiased=False)
    a = (g.view(1, -1) * torch.rsqrt(var + 1e-5).repeat_interleave(Cout // 32, 1))
    ref = Yraw.float() * a.view(B, 1, 1, Cout) + (b.view(1, -1) - mean.repeat_interleave(Cout // 32, 1) * a).view(B, 1, 1, Cout)
    assert rel_err(Y.float(), F.relu(ref)) < OUT_TOL[dtype]
    # the records are the sums of the fp32 accumulators of their 32 rows x cpg columns (the bound test_gpu_ops.py puts on the
    # LayerNorm fold's fp32 row statistics)
    blk = raw.double().reshape(B, -1, 32, 32, Cout // 32)            # [image, block, row, group, channel]
    assert rel_err(rec[..., 0], blk.sum((2, 4))) < 1e-4
    assert rel_err(rec[..., 1], (blk * blk).sum((2, 4))) < 1e-4


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", PLAIN_CASES)
def test_stream_bias_relu_against_fp32(dtype, case):
    X, Wt, bias, _ = operands(dtype, case)
    assert rel_err(run_plain(dtype, case, 16).float(), F.relu(conv32(X, Wt, bias, case[5]))) < OUT_TOL[dtype]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", [c for c in GN_CASES if c[0] == 3])
def test_stream_batch_invariance_bitwise(dtype, case):
    """image 1 of the batch of three == the same image run alone, in output and records"""
    for flags in (0, 16):
        full, one = run_gn(dtype, case, flags), run_gn(dtype, case, flags, image=1)
        for f, o in zip(full, one):
            assert torch.equal(f[1], o[0]), flags
        assert torch.equal(run_plain(dtype, PLAIN_CASES[0], flags)[1], run_plain(dtype, PLAIN_CASES[0], flags, image=1)[0]), flags


def test_stream_whole_forward_equals_tiled_bitwise():
    """Whole forward at B = 2, 384 x 384: with and without the streaming kernel (flag 8) the outputs are the same bits in bf16
    and fp16 -- and in `mixed`, where no launch is eligible and the flag changes nothing."""
    from omnidata_amd.model import DPTDepthModel
    from omnidata_amd.weights import random_state_dict, synthetic_input
    lib = load_library()
    x = synthetic_input(9, 2, "normal").to(DEV)
    try:
        for dtype in ("bf16", "fp16", "mixed"):
            model = DPTDepthModel(num_channels=3, dtype=dtype, max_batch=2)
            model.load_state_dict(random_state_dict(0, 3))
            model.to(DEV)
            outs = []
            for flags in (0, 8, 16):
                lib.dptx_debug_set_gemm_flags(flags)
                outs.append(model(x).clone())
            assert torch.isfinite(outs[0]).all(), dtype
            assert torch.equal(outs[0], outs[1]), dtype
            assert torch.equal(outs[2], outs[1]), dtype
            del model
    finally:
        lib.dptx_debug_set_gemm_flags(0)
