"""Op-level parity of every HIP kernel against a plain PyTorch fp32 reference of the same op on
the same (already 16-bit-rounded) inputs.  Run on an MI355X: pytest -m gpu.
The GEMMs and convolutions are judged element by element against fp64 in tests/test_gpu_gemm_elements.py."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from omnidata_amd.engine import DTYPES, load_library
from tests.gpu_util import (OUT_TOL, TDT, group_max, nhwc_with_group_stats, op_conv, op_gemm, per_group_err, per_row_err, ptr, rel_err,
                            rows_with_stats, stream)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rnd(*shape, dtype="bf16", scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(TDT[dtype]).to(DEV)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (1000, 256, 192), (577 * 3, 768, 768), (18464, 2304, 768),
                                   (4608, 256, 2304), (300, 64, 576), (70000, 64, 64), (5000, 32, 1152), (77, 3072, 768),
                                   (18464, 768, 3072)])  # last: fc2 at B=32 -> 256x256 8-wave tile
def test_gemm_plain(dtype, M, N, K):
    # asymmetric, non-identity operands: a row/col swap or a k-permutation mismatch cannot pass
    A, W = rnd(M, K, dtype=dtype, seed=1), rnd(N, K, dtype=dtype, scale=K ** -0.5, seed=2)
    ref = A.float() @ W.float().t()
    got = op_gemm(dtype, A, W)
    assert rel_err(got.float(), ref) < OUT_TOL[dtype]
    got32 = op_gemm(dtype, A, W, c_fp32=True)
    assert rel_err(got32, ref) < 2e-5


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("M,K", [(1731, 768), (18470, 2048)])  # 2nd: 256x256 8-wave tile (slab epilogue), ragged last m-tile
def test_gemm_epilogues(dtype, M, K):
    N = 768
    A, W = rnd(M, K, dtype=dtype, seed=3), rnd(N, K, dtype=dtype, scale=K ** -0.5, seed=4)
    bias = torch.randn(N, device=DEV)
    R16 = rnd(M, N, dtype=dtype, seed=5)
    R32 = torch.randn(M, N, device=DEV)
    base = A.float() @ W.float().t() + bias
    assert rel_err(op_gemm(dtype, A, W, bias, act=1).float(), F.relu(base)) < OUT_TOL[dtype]
    assert rel_err(op_gemm(dtype, A, W, bias, act=2).float(), F.gelu(base)) < OUT_TOL[dtype]
    assert rel_err(op_gemm(dtype, A, W, bias, R=R16).float(), base + R16.float()) < OUT_TOL[dtype]
    assert rel_err(op_gemm(dtype, A, W, bias, R=R32, c_fp32=True), base + R32) < 2e-5
    # fp32 A operand (ProjectReadout reads the fp32 token stream): rounded to 16-bit while staging
    A32 = torch.randn(M, K, device=DEV)
    ref = A32.to(TDT[dtype]).float() @ W.float().t() + bias
    assert rel_err(op_gemm(dtype, A32, W, bias, c_fp32=True), ref) < 2e-5


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("M,K", [(18464, 768), (18464, 3072), (9232, 768), (1731, 768)])  # proj / fc2 at B = 32, a half batch, a small batch
def test_gemm_token_stream_producer_forms_bitwise(dtype, M, K):
    """proj / fc2 on the 16-bit token stream: C <- C + A W^T + bias IN PLACE plus the LayerNorm fold's row statistics
    (dptx_op_gemm_stream).  Round 6: at B = 32 the launch takes the register-direct epilogue of the 256x256 kernel (residual
    loads up front, the statistics' butterfly replayed across lanes / registers / the two waves of a 128-column block); the
    staged epilogue (debug flag 1) and the one-block-per-tile launch (flag 3) must give the same bits in C AND in the records,
    and both must be right: C against fp32 of the same expression, the records against sums of the fp32 rows.  Two residual
    streams: unit Gaussian rows, and rows with statistics of their own (r in {0, 1, 8}, sigma 2^-6 .. 2^6), where C is checked
    row by row and every record against the sums of its own 128 values."""
    lib = load_library()
    N = 768
    A, W = rnd(M, K, dtype=dtype, seed=11), rnd(N, K, dtype=dtype, scale=K ** -0.5, seed=12)
    bias = torch.randn(N, device=DEV)
    for resid in ("gauss", "rows"):
        C0 = rnd(M, N, dtype=dtype, seed=13) if resid == "gauss" else rows_with_stats(M, N, seed=13)[0].to(TDT[dtype]).to(DEV)
        outs = []
        try:
            for flags in (0, 1, 3):
                lib.dptx_debug_set_gemm_flags(flags)
                C = C0.clone()
                stats = torch.full((M, 8, 2), float("nan"), device=DEV)
                rc = lib.dptx_op_gemm_stream(DTYPES[dtype], ptr(A), ptr(W), ptr(bias), ptr(C), ptr(stats), M, N, K, stream())
                assert rc == 0
                outs.append((C, stats))
        finally:
            lib.dptx_debug_set_gemm_flags(0)
        for C, stats in outs[1:]:
            assert torch.equal(C, outs[0][0])
            assert torch.equal(stats[:, :N // 128], outs[0][1][:, :N // 128])
        C, stats = outs[0]
        ref = A.float() @ W.float().t() + bias + C0.float()
        assert rel_err(C.float(), ref) < OUT_TOL[dtype]
        blk = ref.double().view(M, N // 128, 128)
        assert rel_err(stats[:, :N // 128, 0], blk.sum(2)) < 1e-4        # statistics of the fp32 values, not of the rounded stream
        assert rel_err(stats[:, :N // 128, 1], (blk * blk).sum(2)) < 1e-4
        assert torch.isnan(stats[:, N // 128:]).all()                    # records of blocks the launch does not own stay untouched
        x = stream_ref64(A, W, bias, C0)
        err = per_row_err(C, x)                                           # the stored stream, row by row: rounding is per row
        print(f"\n[16-bit stream {dtype} M={M} K={K} {resid}] worst row err {float(err.max()):.2e}")
        assert (err <= OUT_TOL[dtype]).all(), torch.nonzero(err > OUT_TOL[dtype])[:5, 0].tolist()
        check_records(stats, x)


def stream_ref64(A, W, bias, R):
    """fp64 A W^T + bias + R"""
    return A.double() @ W.double().t() + bias.double() + R.double()


def check_records(stats, x):
    """every record against fp64 sums of its own 128 values of x (fp64 [M, N]): |d sum| <= 1e-4 sum |x|, |d sumsq| <= 1e-4 sum x^2
    (a record of the wrong row or block, or one that misses values, fails however small its row is)"""
    M, N = x.shape
    x = x.view(M, N // 128, 128)
    s1, s2, a1 = x.sum(2), (x * x).sum(2), x.abs().sum(2)
    d1 = (stats[:, :N // 128, 0].double() - s1).abs()
    d2 = (stats[:, :N // 128, 1].double() - s2).abs()
    assert (d1 <= 1e-4 * a1).all(), torch.nonzero(d1 > 1e-4 * a1)[:5].tolist()
    assert (d2 <= 1e-4 * s2).all(), torch.nonzero(d2 > 1e-4 * s2)[:5].tolist()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("M,K", [(18464, 768), (18464, 3072), (1731, 768)])
def test_gemm_fp32_token_stream_producer_forms_bitwise(dtype, M, K):
    """The parity mode's proj / fc2: fp32 stream in place + its 16-bit image + row statistics (dptx_op_gemm_stream32).  These
    launches stay on the staged epilogue (a register-direct form was built in round 6 and measured slower:
    profiles/r06_experiments.md section 8); the launch forms that exist -- persistent tile loop, one block per tile -- must agree
    bit for bit, and be right.  The same two residual streams as the 16-bit test; X checked row by row as well."""
    lib = load_library()
    N = 768
    A, W = rnd(M, K, dtype=dtype, seed=21), rnd(N, K, dtype=dtype, scale=K ** -0.5, seed=22)
    bias = torch.randn(N, device=DEV)
    for resid in ("gauss", "rows"):
        X0 = torch.randn(M, N, device=DEV) if resid == "gauss" else rows_with_stats(M, N, seed=23)[0].to(DEV)
        outs = []
        try:
            for flags in (0, 1, 3):
                lib.dptx_debug_set_gemm_flags(flags)
                X = X0.clone()
                C16 = torch.zeros(M, N, dtype=TDT[dtype], device=DEV)
                stats = torch.full((M, 8, 2), float("nan"), device=DEV)
                rc = lib.dptx_op_gemm_stream32(DTYPES[dtype], ptr(A), ptr(W), ptr(bias), ptr(X), ptr(C16), ptr(stats), M, N, K,
                                               stream())
                assert rc == 0
                outs.append((X, C16, stats))
        finally:
            lib.dptx_debug_set_gemm_flags(0)
        for X, C16, stats in outs[1:]:
            assert torch.equal(X, outs[0][0]) and torch.equal(C16, outs[0][1])
            assert torch.equal(stats[:, :N // 128], outs[0][2][:, :N // 128])
        X, C16, stats = outs[0]
        ref = A.float() @ W.float().t() + bias + X0
        assert rel_err(X, ref) < 2e-5
        assert torch.equal(C16, X.to(TDT[dtype]))                        # the 16-bit image is the rounding of the stored fp32 value
        blk = ref.double().view(M, N // 128, 128)
        assert rel_err(stats[:, :N // 128, 0], blk.sum(2)) < 1e-4
        assert rel_err(stats[:, :N // 128, 1], (blk * blk).sum(2)) < 1e-4
        x = stream_ref64(A, W, bias, X0)
        err = per_row_err(X, x)
        print(f"\n[fp32 stream {dtype} M={M} K={K} {resid}] worst row err {float(err.max()):.2e}")
        assert (err <= 2e-5).all(), torch.nonzero(err > 2e-5)[:5, 0].tolist()
        check_records(stats, x)


def conv_ref(X, Wt, bias, stride, pad_t, pad_l, Ho, Wo, a_relu):
    x = X.float().permute(0, 3, 1, 2)
    if a_relu:
        x = F.relu(x)
    k = Wt.shape[1]
    H, W = x.shape[-2:]
    pb = max((Ho - 1) * stride + k - H - pad_t, 0)
    pr = max((Wo - 1) * stride + k - W - pad_l, 0)
    x = F.pad(x, [pad_l, pr, pad_t, pb])
    y = F.conv2d(x, Wt.float().permute(0, 3, 1, 2), bias, stride)
    assert y.shape[-2:] == (Ho, Wo)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", [
    # B, H, Cin, Cout, k, stride, pad_t, Ho, a_relu, act, residual
    (2, 24, 256, 256, 3, 1, 1, 24, 1, 1, False),   # RCU conv1: pre-ReLU + ReLU epilogue
    (2, 24, 256, 256, 3, 1, 1, 24, 0, 0, True),    # RCU conv2: + residual
    (3, 48, 128, 128, 3, 2, 0, 24, 0, 0, False),   # bottleneck conv2 stride 2, TF-SAME pad (0,1)
    (2, 48, 256, 512, 1, 2, 0, 24, 0, 0, False),   # downsample 1x1 stride 2
    (1, 24, 768, 768, 3, 2, 1, 12, 0, 0, False),   # act_postprocess4 conv 3x3 s2 p1
    (2, 96, 64, 64, 3, 1, 1, 96, 0, 0, False),     # stage0 conv2 (N=64)
    (1, 40, 128, 32, 3, 1, 1, 40, 0, 1, False),    # head conv 128->32 (+ReLU), N=32 tile
    (5, 12, 768, 256, 3, 1, 1, 12, 0, 0, False),   # layer4_rn (small map, K=6912)
    (8, 96, 256, 256, 3, 1, 1, 96, 1, 1, False),   # big-M RCU conv1: 256x256 8-wave tile, pre-ReLU
    (8, 96, 256, 128, 3, 1, 1, 96, 0, 0, True),    # big-M, N=128, residual
    (9, 48, 512, 256, 3, 1, 1, 48, 0, 0, False),   # layer2_rn at batch 9 (M not a multiple of 256)
    (25, 48, 256, 256, 3, 1, 1, 48, 1, 0, True),   # 256x256 tile, M = 57600 (225 m-tiles), pre-ReLU + residual
])
def test_conv_implicit_gemm(dtype, case):
    B, H, Cin, Cout, k, stride, pad, Ho, a_relu, act, res = case
    X = rnd(B, H, H, Cin, dtype=dtype, seed=6)
    Wt = rnd(Cout, k, k, Cin, dtype=dtype, scale=(k * k * Cin) ** -0.5, seed=7)
    bias = torch.randn(Cout, device=DEV) * 0.1
    R = rnd(B, Ho, Ho, Cout, dtype=dtype, seed=8) if res else None
    ref = conv_ref(X, Wt, bias, stride, pad, pad, Ho, Ho, a_relu)
    if act == 1:
        ref = F.relu(ref)
    if res:
        ref = ref + R.float()
    got = op_conv(dtype, X, Wt, bias, R, stride, pad, pad, Ho, Ho, a_relu, act)
    assert rel_err(got.float(), ref) < OUT_TOL[dtype]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,S", [(1, 577), (3, 577), (2, 64), (1, 200), (2, 65), (1, 66), (2, 17), (1, 129)])
def test_attention(dtype, B, S):
    lib = load_library()
    H = 12
    qkv = rnd(B * S, 3 * H * 64, dtype=dtype, seed=9)
    # spike a few keys so the running max really jumps between tiles (online-softmax rescale path)
    q3 = qkv.view(B, S, 3, H, 64)
    q3[:, S // 2, 1] *= 6.0
    q3[:, S - 1, 1] *= 4.0
    q3[0, 0, 1, ::2] *= 5.0   # key 0 (the cls token) is handled outside the key tiles: make it dominate for some heads
    out = torch.empty(B * S, H * 64, device=DEV, dtype=TDT[dtype])
    assert lib.dptx_op_attention(DTYPES[dtype], ptr(qkv), ptr(out), B, S, H, stream()) == 0
    q, k, v = [t.permute(0, 2, 1, 3).float() for t in q3.unbind(2)]
    att = ((q @ k.transpose(-1, -2)) * 0.125).softmax(-1)
    ref = (att @ v).permute(0, 2, 1, 3).reshape(B * S, H * 64)
    # P is rounded to 16 bit before the PV product: allow 2x the output-rounding budget
    assert rel_err(out.float(), ref) < 2 * OUT_TOL[dtype]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_layernorm(dtype):
    lib = load_library()
    M, C = 1155, 768
    x = torch.randn(M, C, device=DEV) * 3 + 0.7
    g, b = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    y = torch.empty(M, C, device=DEV, dtype=TDT[dtype])
    assert lib.dptx_op_layernorm(DTYPES[dtype], ptr(x), ptr(g), ptr(b), ptr(y), M, C, 1e-6, stream()) == 0
    assert rel_err(y.float(), F.layer_norm(x, (C,), g, b, 1e-6)) < OUT_TOL[dtype]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,HW,C,relu,res", [(2, 9216, 64, 1, False), (2, 2304, 128, 1, False), (3, 576, 1024, 1, True),
                                              (1, 36864, 64, 0, False), (2, 9216, 256, 1, True), (2, 2304, 512, 0, False)])
def test_groupnorm(dtype, B, HW, C, relu, res):
    lib = load_library()
    X = rnd(B, HW, C, dtype=dtype, seed=10) * 2 + 0.5
    X = X.to(TDT[dtype])
    g, b = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    R = rnd(B, HW, C, dtype=dtype, seed=11) if res else None
    Y = torch.empty_like(X)
    scratch = torch.empty(B * 144 * 64, device=DEV)
    assert lib.dptx_op_groupnorm(DTYPES[dtype], ptr(X), ptr(g), ptr(b), ptr(R), ptr(Y), B, HW, C, relu, 1e-5, ptr(scratch), stream()) == 0
    ref = F.group_norm(X.float().permute(0, 2, 1), 32, g, b, 1e-5).permute(0, 2, 1)
    if res:
        ref = ref + R.float()
    if relu:
        ref = F.relu(ref)
    assert rel_err(Y.float(), ref) < OUT_TOL[dtype]


# (B, H, Cin, Cout, k, stride, pad, Ho, residual): every tile shape the ResNetV2 stage convs take, incl. a ragged last
# m-tile (B*Ho*Ho not a multiple of the tile), images that end inside a tile (576 rows), cpg from 2 to 32
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", [(2, 96, 64, 64, 1, 1, 0, 96, False), (3, 24, 256, 1024, 1, 1, 0, 24, True),
                                  (3, 24, 256, 256, 3, 1, 1, 24, False), (2, 48, 128, 512, 1, 1, 0, 48, True),
                                  (1, 96, 128, 128, 3, 2, 0, 48, False), (5, 24, 1024, 256, 1, 1, 0, 24, False),
                                  (32, 24, 512, 256, 1, 1, 0, 24, False)])
def test_conv_groupnorm_fused_stats(dtype, case):
    """GroupNorm statistics out of the conv's GEMM epilogue (what the ResNetV2 stages run) against conv -> group_norm."""
    lib = load_library()
    B, H, Cin, Cout, k, stride, pad, Ho, res = case
    X = rnd(B, H, H, Cin, dtype=dtype, seed=20)
    Wt = rnd(Cout, k, k, Cin, dtype=dtype, scale=(k * k * Cin) ** -0.5, seed=21)
    g, b = torch.randn(Cout, device=DEV), torch.randn(Cout, device=DEV)
    R = rnd(B, Ho, Ho, Cout, dtype=dtype, seed=22) if res else None
    Yraw = torch.empty(B, Ho, Ho, Cout, device=DEV, dtype=TDT[dtype])
    Y = torch.empty_like(Yraw)
    scratch = torch.zeros(B * (Ho * Ho // 32) * 64, device=DEV)
    rc = lib.dptx_op_conv_groupnorm(DTYPES[dtype], ptr(X), ptr(Wt), ptr(Yraw), ptr(g), ptr(b), ptr(R), ptr(Y), B, H, H, Cin,
                                    Cout, k, stride, pad, pad, Ho, Ho, 1, 1e-5, ptr(scratch), stream())
    assert rc == 0
    raw = conv_ref(X, Wt, None, stride, pad, pad, Ho, Ho, 0)          # fp32 conv of the 16-bit operands, NHWC
    assert rel_err(Yraw.float(), raw) < OUT_TOL[dtype]
    # the statistics are those of the fp32 accumulators; the apply pass normalises the stored (rounded) map
    xr = raw.permute(0, 3, 1, 2).reshape(B, 32, -1)
    mean, var = xr.mean(-1), xr.var(-1, unbiased=False)
    a = (g.view(1, -1) * torch.rsqrt(var + 1e-5).repeat_interleave(Cout // 32, 1))
    ref = Yraw.float() * a.view(B, 1, 1, Cout) + (b.view(1, -1) - mean.repeat_interleave(Cout // 32, 1) * a).view(B, 1, 1, Cout)
    if res:
        ref = ref + R.float()
    ref = F.relu(ref)
    assert rel_err(Y.float(), ref) < OUT_TOL[dtype]
    # batch invariance, bit for bit: image i of the batch == image i alone
    i = B - 1
    Y1 = torch.empty(1, Ho, Ho, Cout, device=DEV, dtype=TDT[dtype])
    R1 = R[i:i + 1].contiguous() if res else None
    rc = lib.dptx_op_conv_groupnorm(DTYPES[dtype], ptr(X[i:i + 1].contiguous()), ptr(Wt), ptr(Y1), ptr(g), ptr(b), ptr(R1), ptr(Y1),
                                    1, H, H, Cin, Cout, k, stride, pad, pad, Ho, Ho, 1, 1e-5, ptr(scratch), stream())
    assert rc == 0
    assert torch.equal(Y1[0], Y[i])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,C", [(2, 12, 256), (1, 96, 256), (2, 48, 128)])
def test_upsample2x_align_corners(dtype, B, H, C):
    lib = load_library()
    X = rnd(B, H, H, C, dtype=dtype, seed=12)
    Y = torch.empty(B, 2 * H, 2 * H, C, device=DEV, dtype=TDT[dtype])
    assert lib.dptx_op_upsample2x(DTYPES[dtype], ptr(X), ptr(Y), B, H, H, C, stream()) == 0
    ref = F.interpolate(X.float().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    assert rel_err(Y.float(), ref) < OUT_TOL[dtype]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,W", [(2, 384, 384), (1, 64, 128), (3, 96, 256), (2, 256, 320), (1, 96, 160), (1, 64, 96)])
def test_fused_stem_conv(dtype, B, H, W):
    """7x7 stride-2 TF-SAME conv straight from the NCHW fp32 image (no im2col).  One number per tensor on positive images of one
    scale: tests/test_gpu_stem_elements.py judges every element of this kernel, in all four modes, against fp64."""
    lib = load_library()
    x = torch.rand(B, 3, H, W, device=DEV)
    w = torch.randn(64, 3, 7, 7, device=DEV) * 147 ** -0.5
    wp = torch.zeros(64, 176, device=DEV)
    wp[:, :168].view(64, 3, 7, 8)[..., :7] = w                   # k = (c*7 + ky)*8 + kx
    wp = wp.to(TDT[dtype])
    y = torch.empty(B, H // 2, W // 2, 64, device=DEV, dtype=TDT[dtype])
    assert lib.dptx_op_stem_conv(DTYPES[dtype], ptr(x), ptr(wp), ptr(y), B, H, W, stream()) == 0
    ref = F.conv2d(F.pad(x.to(TDT[dtype]).float(), [2, 3, 2, 3]), w.to(TDT[dtype]).float(), None, 2).permute(0, 2, 3, 1)
    assert ref.shape == y.shape
    assert rel_err(y.float(), ref) < OUT_TOL[dtype]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,Hs,Ws,C,relu", [(2, 48, 64, 3, 1), (1, 192, 192, 1, 1), (3, 32, 48, 3, 0), (5, 16, 16, 2, 1)])
def test_fused_head_tail(dtype, B, Hs, Ws, C, relu):
    """x2 bilinear (align_corners) -> conv3x3 128->32 -> ReLU -> conv1x1 32->C -> ReLU in one kernel (head.hip), against
    the same chain in fp32 torch on the same 16-bit inputs (the up-sampled map rounded to 16 bit, as the kernel does)."""
    lib = load_library()
    H0 = rnd(B, Hs, Ws, 128, dtype=dtype, seed=21)
    W2 = rnd(32, 3, 3, 128, dtype=dtype, scale=1152 ** -0.5, seed=22)
    b2 = torch.randn(32, device=DEV) * 0.3
    w4 = torch.randn(C, 32, device=DEV) * 0.3
    b4 = torch.randn(C, device=DEV) * 0.2
    y = torch.full((B, C, 2 * Hs, 2 * Ws), float("nan"), device=DEV)
    assert lib.dptx_op_head_tail(DTYPES[dtype], ptr(H0), ptr(W2), ptr(b2), ptr(w4), ptr(b4), ptr(y), B, Hs, Ws, C, relu, stream()) == 0
    up = F.interpolate(H0.float().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
    up = up.to(TDT[dtype]).float()
    h = F.relu(F.conv2d(up, W2.float().permute(0, 3, 1, 2), b2, padding=1))
    ref = F.conv2d(h, w4.view(C, 32, 1, 1), b4)
    if relu:
        ref = F.relu(ref)
    assert torch.isfinite(y).all()
    # a 16-bit rounding of the up-sampled map can flip where the two fp32 interpolation formulas differ in the last bit
    assert rel_err(y, ref) < 2e-3 * (1 if dtype == "bf16" else 0.2)
    # and against this library's own unfused kernels the result is the same up to fp32 summation order
    U = torch.empty(B, 2 * Hs, 2 * Ws, 128, device=DEV, dtype=TDT[dtype])
    assert lib.dptx_op_upsample2x(DTYPES[dtype], ptr(H0), ptr(U), B, Hs, Ws, 128, stream()) == 0
    h2 = F.relu(F.conv2d(U.float().permute(0, 3, 1, 2), W2.float().permute(0, 3, 1, 2), b2, padding=1))
    ref2 = F.conv2d(h2, w4.view(C, 32, 1, 1), b4)
    if relu:
        ref2 = F.relu(ref2)
    assert rel_err(y, ref2) < 2e-5


# ------------------------------------------------------------------------------------------------------------------------------
# Normalisation statistics on inputs whose statistics differ row by row and (image, group) by (image, group)
# (tests/gpu_util.py rows_with_stats / nhwc_with_group_stats).  Errors are measured per row / per (image, group), relative to
# that row's / group's own max |ref|: with sigmas spread over 2^12 one error against the global max would hide every small row.
U32 = 2.0 ** -24        # fp32 unit roundoff
STEP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}   # unit roundoff of the 16-bit types


def ln_row_bar(tol, r):
    """Per-row bar of the LayerNorm kernel: the output tolerance plus the fp32 mean's error.  The kernel sums C values of
    magnitude <= |mu| + 4 sigma along at most 4 VPL + 6 <= 22 rounded additions (lane partials, then the butterfly), so
    |d mean| <= 22 u (|mu| + 4 sigma) and the normalised output moves by |d mean| / sigma = 22 u (r + 4) -- negligible at
    r <= 8, 1.5e-3 for the near-constant row (r = 1000) that every test input carries."""
    return tol + 22 * U32 * (r + 4)


LN_FAMILIES = {"r018": dict(r_values=(0.0, 1.0, 8.0)), "outliers": dict(r_values=(0.0, 1.0), outliers=True)}


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("C", [768, 1024])
@pytest.mark.parametrize("family", list(LN_FAMILIES))
def test_layernorm_per_row_statistics(dtype, C, family):
    """dptx_op_layernorm with every row on its own (mean, sigma): M = 1155 is not a multiple of the 4 rows per block; C = 1024 is
    DPT-Large's width (the VPL = 4 instantiation).  Against fp64 F.layer_norm of the same fp32 rows, row by row."""
    lib = load_library()
    M = 1155
    x, r = rows_with_stats(M, C, seed=40 + C, **LN_FAMILIES[family])
    x = x.to(DEV)
    g, b = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    y = torch.full((M + 1, C), float("nan"), device=DEV, dtype=TDT[dtype])
    assert lib.dptx_op_layernorm(DTYPES[dtype], ptr(x), ptr(g), ptr(b), ptr(y), M, C, 1e-6, stream()) == 0
    ref = F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-6)
    err = per_row_err(y[:M], ref).cpu()
    bar = ln_row_bar(OUT_TOL[dtype], r)
    print(f"\n[layernorm {dtype} C={C} {family}] worst row err / bar {float((err / bar).max()):.3f}")
    assert (err <= bar).all(), [(int(m), float(err[m]), float(r[m])) for m in torch.nonzero(err > bar)[:5, 0]]
    assert torch.isnan(y[M].float()).all()                           # the row after the last one is not written


GN_CASES = [  # (B, HW, C, relu, res): spv = 4 / 2 / 1 (C = 64 / 128 / >= 256); HW not a multiple of the chunk (16384 / C px)
    (3, 777, 64, 1, False), (3, 300, 128, 0, True), (4, 200, 256, 1, True), (3, 90, 1024, 0, False), (3, 1000, 512, 1, False)]


def groupnorm_ref(X, g, b, R, relu):
    """fp64 GroupNorm(32) of the stored NHWC input (+ R, + ReLU)."""
    ref = F.group_norm(X.double().permute(0, 2, 1), 32, g.double(), b.double(), 1e-5).permute(0, 2, 1)
    if R is not None:
        ref = ref + R.double()
    return F.relu(ref) if relu else ref


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,HW,C,relu,res", GN_CASES)
def test_groupnorm_per_group_statistics(dtype, B, HW, C, relu, res):
    """dptx_op_groupnorm with every (image, group) on its own (mean, sigma), checked group by group: a kernel that mixes up
    which channels belong to which group (the three slot paths of gn_stats_kernel), or which image a record belongs to, fails."""
    lib = load_library()
    X = nhwc_with_group_stats(B, HW, C, seed=50 + C).to(TDT[dtype]).to(DEV)
    g, b = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    R = rnd(B, HW, C, dtype=dtype, seed=51) if res else None
    Y = torch.empty_like(X)
    pix = min(max(16384 // C, 16), 256)
    scratch = torch.empty(B * ((HW + pix - 1) // pix) * 64, device=DEV)
    assert lib.dptx_op_groupnorm(DTYPES[dtype], ptr(X), ptr(g), ptr(b), ptr(R), ptr(Y), B, HW, C, relu, 1e-5, ptr(scratch),
                                 stream()) == 0
    err = per_group_err(Y, groupnorm_ref(X, g, b, R, relu), scale=group_max(groupnorm_ref(X, g, b, R, 0)))
    print(f"\n[groupnorm {dtype} B={B} HW={HW} C={C}] worst (image, group) err {float(err.max()):.2e}")
    assert (err < OUT_TOL[dtype]).all(), torch.nonzero(err >= OUT_TOL[dtype])[:5].tolist()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", [(3, 96, 64, 64, 1, 1, 0, 96, False), (3, 24, 256, 256, 3, 1, 1, 24, False),
                                  (3, 48, 128, 512, 1, 1, 0, 48, True), (3, 96, 128, 128, 3, 2, 0, 48, False)])
def test_conv_groupnorm_per_group_statistics(dtype, case):
    """dptx_op_conv_groupnorm with statistics of its own for every output group and every image: the weight rows of group g are
    scaled by 2^((5 g) % 7 - 3) and shifted by a per-group offset (the input is positive, so the offset moves the group's mean),
    and image i of X is scaled by 2^(i - 1).  The assertions of test_conv_groupnorm_fused_stats, but per (image, group)."""
    lib = load_library()
    B, H, Cin, Cout, k, stride, pad, Ho, res = case
    cpg = Cout // 32
    X = (rnd(B, H, H, Cin, dtype=dtype, seed=60).float().abs() + 0.25) * torch.exp2(torch.arange(B, device=DEV) - 1.0).view(B, 1, 1, 1)
    X = X.to(TDT[dtype])
    grp = torch.arange(Cout, device=DEV) // cpg
    scale = torch.exp2(((5 * grp) % 7 - 3).float())
    offset = torch.where(grp % 2 == 0, 1.0, -1.0) * (0.5 + (grp % 3).float()) * (k * k * Cin) ** -0.5
    Wt = (rnd(Cout, k, k, Cin, dtype=dtype, scale=(k * k * Cin) ** -0.5, seed=61).float() + offset.view(-1, 1, 1, 1)) * scale.view(-1, 1, 1, 1)
    Wt = Wt.to(TDT[dtype])
    g, b = torch.randn(Cout, device=DEV), torch.randn(Cout, device=DEV)
    R = rnd(B, Ho, Ho, Cout, dtype=dtype, seed=62) if res else None
    Yraw = torch.empty(B, Ho, Ho, Cout, device=DEV, dtype=TDT[dtype])
    Y = torch.empty_like(Yraw)
    scratch = torch.zeros(B * (Ho * Ho // 32) * 64, device=DEV)
    rc = lib.dptx_op_conv_groupnorm(DTYPES[dtype], ptr(X), ptr(Wt), ptr(Yraw), ptr(g), ptr(b), ptr(R), ptr(Y), B, H, H, Cin,
                                    Cout, k, stride, pad, pad, Ho, Ho, 1, 1e-5, ptr(scratch), stream())
    assert rc == 0
    raw = conv_ref(X.double(), Wt.double(), None, stride, pad, pad, Ho, Ho, 0)      # fp64 conv of the 16-bit operands, NHWC
    assert (per_group_err(Yraw.reshape(B, -1, Cout), raw.reshape(B, -1, Cout)) < OUT_TOL[dtype]).all()
    # the statistics are those of the (fp32) accumulators; the apply pass normalises the stored (rounded) map
    xr = raw.permute(0, 3, 1, 2).reshape(B, 32, -1)
    mean, var = xr.mean(-1), xr.var(-1, unbiased=False)
    a = g.double().view(1, -1) * torch.rsqrt(var + 1e-5).repeat_interleave(cpg, 1)
    ref = Yraw.double() * a.view(B, 1, 1, Cout) + (b.double().view(1, -1) - mean.repeat_interleave(cpg, 1) * a).view(B, 1, 1, Cout)
    if res:
        ref = ref + R.double()
    scale = group_max(ref.reshape(B, -1, Cout))                        # before the ReLU
    ref = F.relu(ref)
    err = per_group_err(Y.reshape(B, -1, Cout), ref.reshape(B, -1, Cout), scale=scale)
    print(f"\n[conv+groupnorm {dtype} {case}] worst (image, group) err {float(err.max()):.2e}")
    assert (err < OUT_TOL[dtype]).all(), torch.nonzero(err >= OUT_TOL[dtype])[:5].tolist()
    i = B - 1                                                          # batch invariance, bit for bit
    Y1 = torch.empty(1, Ho, Ho, Cout, device=DEV, dtype=TDT[dtype])
    R1 = R[i:i + 1].contiguous() if res else None
    rc = lib.dptx_op_conv_groupnorm(DTYPES[dtype], ptr(X[i:i + 1].contiguous()), ptr(Wt), ptr(Y1), ptr(g), ptr(b), ptr(R1), ptr(Y1),
                                    1, H, H, Cin, Cout, k, stride, pad, pad, Ho, Ho, 1, 1e-5, ptr(scratch), stream())
    assert rc == 0
    assert torch.equal(Y1[0], Y[i])


def maxpool_same_ref(y):
    """timm MaxPool2dSame(3, 2) of NHWC y: -inf padding (0, 1, 0, 1) for even sizes, then max_pool2d(3, 2)."""
    t = F.pad(y.permute(0, 3, 1, 2), [0, 1, 0, 1], value=float("-inf"))
    return F.max_pool2d(t, 3, 2).permute(0, 2, 3, 1)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,W", [(1, 192, 192), (3, 32, 48), (2, 144, 224), (3, 64, 96)])
def test_gn_relu_maxpool_per_group_statistics(dtype, B, H, W):
    """The stem's GroupNorm + ReLU + MaxPool2dSame(3, 2) (gn_relu_maxpool_kernel) at the 384 stem (192 x 192 x 64), flex stems
    and B = 3, every (image, group) on its own statistics, against timm's module order in fp64, per (image, group).  Every
    single element, with window taps of different sizes, is judged in tests/test_gpu_stem_elements.py."""
    lib = load_library()
    C = 64
    X = nhwc_with_group_stats(B, H * W, C, seed=70 + H).to(TDT[dtype]).to(DEV).view(B, H, W, C)
    g, b = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    scratch = torch.empty(B * ((H * W + 255) // 256) * 64, device=DEV)
    Y = torch.full((B, H // 2, W // 2, C), float("nan"), device=DEV, dtype=TDT[dtype])
    assert lib.dptx_op_gn_relu_maxpool(DTYPES[dtype], ptr(X), ptr(g), ptr(b), ptr(Y), B, H, W, C, 1e-5, ptr(scratch), stream()) == 0
    y = groupnorm_ref(X.view(B, H * W, C), g, b, None, 0)
    ref = maxpool_same_ref(F.relu(y).view(B, H, W, C))
    assert ref.shape == Y.shape
    err = per_group_err(Y.view(B, -1, C), ref.reshape(B, -1, C), scale=group_max(y))
    print(f"\n[gn+relu+maxpool {dtype} B={B} {H}x{W}] worst (image, group) err {float(err.max()):.2e}")
    assert (err < OUT_TOL[dtype]).all(), torch.nonzero(err >= OUT_TOL[dtype])[:5].tolist()


@pytest.mark.parametrize("H,W", [(33, 48), (32, 47), (31, 31)])
def test_gn_relu_maxpool_rejects_odd_sizes(H, W):
    """The kernel pads (0, 1); SAME padding of an odd size is (1, 1).  launch_gn_relu_maxpool -- the guard the forward relies on;
    the op entry point runs the statistics pass and then calls it -- refuses odd sizes instead of computing a wrong result, and
    writes no output."""
    lib = load_library()
    B, C = 1, 64
    X = rnd(B, H, W, C, seed=71)
    g, b = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    scratch = torch.empty(B * ((H * W + 255) // 256) * 64, device=DEV)
    Y = torch.full((B, (H + 1) // 2, (W + 1) // 2, C), float("nan"), device=DEV, dtype=torch.bfloat16)
    assert lib.dptx_op_gn_relu_maxpool(DTYPES["bf16"], ptr(X), ptr(g), ptr(b), ptr(Y), B, H, W, C, 1e-5, ptr(scratch), stream()) != 0
    torch.cuda.synchronize()
    assert torch.isnan(Y.float()).all()


# ------------------------------------------------------------------------------------------------- the LayerNorm fold, op level
def ln_records(x):
    """(sum, sum of squares) records of the fp32 rows x [M, K] per 128-column block, in fp64 rounded to fp32, as the producers
    write them: [M, 8, 2] with the slots past K / 128 NaN (a launch that reads them turns the row into NaN)."""
    M, K = x.shape
    nb = K // 128
    blk = x.double().view(M, nb, 128)
    rec = torch.full((M, 8, 2), float("nan"), device=x.device)
    rec[:, :nb, 0] = blk.sum(2).float()
    rec[:, :nb, 1] = (blk * blk).sum(2).float()
    return rec


def gemm_ln(dtype, A, W, bias, rec, colsum, act, eps=1e-6):
    lib = load_library()
    M, K = A.shape
    N = W.shape[0]
    C = torch.full((M, N), float("nan"), device=DEV, dtype=TDT[dtype])
    assert lib.dptx_op_gemm_ln(DTYPES[dtype], ptr(A), ptr(W), ptr(bias), ptr(C), M, N, K, act, ptr(rec), ptr(colsum), K // 128, eps,
                               stream()) == 0
    return C


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("N,K", [(2304, 768), (3072, 768), (3072, 1024), (4096, 1024)])   # qkv / fc1 of ViT-B and of ViT-L
@pytest.mark.parametrize("M", [577, 1731, 18464])    # 1 and 3 images (ragged m-tiles), B = 32 (256x256 persistent kernel)
def test_gemm_ln_consumer_epilogue(dtype, N, K, M):
    """dptx_op_gemm_ln -- the qkv / fc1 launch of every ViT block under the LayerNorm fold -- against fp64 of exactly its formula,
    y = act((A W^T - mu colsum) rstd + bias), on the same 16-bit operands, with (mu, rstd) from the same fp32 records
    (mu = S / K, rstd = (Q / K - mu^2 + eps)^-1/2 of the record sums S, Q).  Rows carry statistics of their own (r = |mu| / sigma
    in {0, 1, 8}, sigmas over 2^12; outliers at M = 577); record slots the launch must not read are NaN.

    Bar, element by element (u = 2^-24, s = unit roundoff of the 16-bit output):
      |y - ref| <= 1.25 (s |ref| + 1.13 (rstd E_acc + |pre| e_rstd)) + 2^-24,
      E_acc  = 4 u sqrt(K) sum_k |A_mk W_nk|  + |colsum_n| u (8 sum_j |S_j| / K + 2 |mu|)  -- fp32 accumulation of A W^T (random
               walk over K roundings) and the fp32 mu (record combine, the 1 / K factor) times colsum: this is the (1 + r) term,
               since sum_k |A_mk W_nk| ~ (|mu| + sigma) |W_n|_1;
      e_rstd = u (8 (1 + r)^2 + 4)  -- the single-pass variance Q / K - mu^2 from fp32 record sums loses u (1 + r^2) relative;
      1.13 = max |gelu'|; the 1.25 covers the fused multiply-adds, the bias add and the erf approximation.
    The three launch forms of the 256x256 kernel (dptx_debug_set_gemm_flags 0 / 1 / 3) must give the same bits."""
    lib = load_library()
    x, _ = rows_with_stats(M, K, r_values=(0.0, 1.0, 8.0), outliers=(M == 577), near_constant=False, seed=80 + M + K)
    x = x.to(DEV)
    A = x.to(TDT[dtype])
    W = rnd(N, K, dtype=dtype, scale=K ** -0.5, seed=81)
    bias = torch.randn(N, device=DEV)
    colsum = W.double().sum(1).float()
    rec = ln_records(x)
    S, Q = rec[:, :K // 128, 0].double().sum(1), rec[:, :K // 128, 1].double().sum(1)
    mu = S / K
    var = Q / K - mu * mu
    rstd = (var + 1e-6).rsqrt()
    r = mu.abs() / var.sqrt()
    Ad, Wd = A.double(), W.double()
    acc = Ad @ Wd.t()
    core = (acc - mu.view(-1, 1) * colsum.double().view(1, -1)) * rstd.view(-1, 1)
    e_acc = 4 * U32 * math.sqrt(K) * (Ad.abs() @ Wd.abs().t())
    e_acc += colsum.double().abs().view(1, -1) * U32 * (8 * rec[:, :K // 128, 0].double().abs().sum(1) / K + 2 * mu.abs()).view(-1, 1)
    e_pre = rstd.view(-1, 1) * e_acc + core.abs() * (U32 * (8 * (1 + r) ** 2 + 4)).view(-1, 1)
    del e_acc, acc
    for act in (0, 2):
        pre = core + bias.double()
        ref = F.gelu(pre) if act == 2 else pre
        forms = []
        try:
            for flags in (0, 1, 3):
                lib.dptx_debug_set_gemm_flags(flags)
                forms.append(gemm_ln(dtype, A, W, bias, rec, colsum, act))
        finally:
            lib.dptx_debug_set_gemm_flags(0)
        for Cf in forms[1:]:
            assert torch.equal(Cf, forms[0])
        got = forms[0]
        assert torch.isfinite(got.float()).all()
        bar = 1.25 * (STEP[dtype] * ref.abs() + 1.13 * e_pre) + 2.0 ** -24
        ratio = ((got.double() - ref).abs() / bar).amax(1)
        print(f"\n[gemm_ln {dtype} M={M} N={N} K={K} act={act}] worst |err| / bar {float(ratio.max()):.3f}, rows' rel err "
              f"{float(per_row_err(got, ref).max()):.2e}")
        assert (ratio <= 1).all(), [(int(m), float(ratio[m]), float(r[m])) for m in torch.nonzero(ratio > 1)[:5, 0]]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("C", [768, 1024])
def test_cls_rows(dtype, C):
    """dptx_op_cls_rows (launch_cls_rows, 256 threads per block at C = 768, 1024 at C = 1024): row b S of the fp32 stream = cls +
    pos[0], its 16-bit copy, its records (fp32 sums per 128-column block, against fp64 sums of the row) and its e4m3 copy; every
    other row of every output stays untouched."""
    lib = load_library()
    B, S = 3, 9
    gen = torch.Generator().manual_seed(90 + C)
    cls = (torch.randn(C, generator=gen) * 0.3 + 2.0).to(DEV)              # a row with a mean: r ~ 7
    pos = (torch.randn(C, generator=gen) * torch.linspace(0.01, 4.0, C)).to(DEV)
    q = 4.0
    X = torch.full((B * S, C), float("nan"), device=DEV)
    X16 = torch.full((B * S, C), float("nan"), device=DEV, dtype=TDT[dtype])
    rec = torch.full((B * S, 8, 2), float("nan"), device=DEV)
    X8 = torch.full((B * S, C), 0x7F, device=DEV, dtype=torch.uint8)     # 0x7f: e4m3 NaN
    assert lib.dptx_op_cls_rows(DTYPES[dtype], ptr(cls), ptr(pos), ptr(X), B, S, C, ptr(X16), ptr(rec), ptr(X8), q, stream()) == 0
    v = cls + pos                                                          # one fp32 add, as the kernel does
    rows = torch.arange(B) * S
    other = torch.ones(B * S, dtype=torch.bool)
    other[rows] = False
    for b in range(B):
        m = b * S
        assert torch.equal(X[m], v)
        assert torch.equal(X16[m], v.to(TDT[dtype]))
        blk = v.double().view(C // 128, 128)
        assert ((rec[m, :C // 128, 0].double() - blk.sum(1)).abs() <= 1e-6 * blk.abs().sum(1)).all()
        assert ((rec[m, :C // 128, 1].double() - (blk * blk).sum(1)).abs() <= 1e-6 * (blk * blk).sum(1)).all()
        assert torch.isnan(rec[m, C // 128:]).all()
        want8 = (v * q).clamp(-448, 448).to(torch.float8_e4m3fn)
        assert torch.equal(X8[m].view(torch.float8_e4m3fn).float(), want8.float())
    assert torch.isnan(X[other]).all() and torch.isnan(X16[other].float()).all() and torch.isnan(rec[other]).all()
    assert (X8[other] == 0x7F).all()
    # records have a row stride of 8: a row wider than 1024 with records is refused (nothing is launched)
    assert lib.dptx_op_cls_rows(DTYPES[dtype], ptr(cls), ptr(pos), None, 1, S, 1152, None, ptr(rec), None, q, stream()) != 0


def fold_vs_separate(dtype, x, N=2304):
    """The LayerNorm fold's chain (producer records + 16-bit copy -> dptx_op_gemm_ln with W' = gamma (.) W, b' = b + W beta and
    colsum of the rounded W', as the engine packs them) and the unfused chain (dptx_op_layernorm -> dptx_op_gemm) on the fp32
    rows x [M, K]; returns (fold, separate, fp64 F.linear(F.layer_norm(x)))."""
    lib = load_library()
    M, K = x.shape
    gen = torch.Generator().manual_seed(95)
    W32 = (torch.randn(N, K, generator=gen) * K ** -0.5).to(DEV)
    b = (torch.randn(N, generator=gen) * 0.1).to(DEV)
    gamma = (1.0 + 0.3 * torch.randn(K, generator=gen)).to(DEV)
    beta = (0.2 * torch.randn(K, generator=gen)).to(DEV)
    # producer: the parity mode's fp32 stream launch with a zero product -- X <- X + 0, its 16-bit image, its records
    Z = torch.zeros(M, 64, device=DEV, dtype=TDT[dtype])
    Wz = torch.zeros(K, 64, device=DEV, dtype=TDT[dtype])
    X = x.clone()
    X16 = torch.empty(M, K, device=DEV, dtype=TDT[dtype])
    rec = torch.full((M, 8, 2), float("nan"), device=DEV)
    assert lib.dptx_op_gemm_stream32(DTYPES[dtype], ptr(Z), ptr(Wz), None, ptr(X), ptr(X16), ptr(rec), M, K, 64, stream()) == 0
    assert torch.equal(X, x) and torch.equal(X16, x.to(TDT[dtype]))
    Wf = (W32 * gamma.view(1, -1)).to(TDT[dtype])
    bf = (b.double() + W32.double() @ beta.double()).float()
    colsum = Wf.double().sum(1).float()
    fold = gemm_ln(dtype, X16, Wf, bf, rec, colsum, 0)
    # unfused: LayerNorm to 16 bit, then the plain GEMM on the rounded W
    y16 = torch.empty(M, K, device=DEV, dtype=TDT[dtype])
    assert lib.dptx_op_layernorm(DTYPES[dtype], ptr(x), ptr(gamma), ptr(beta), ptr(y16), M, K, 1e-6, stream()) == 0
    sep = op_gemm(dtype, y16, W32.to(TDT[dtype]), b)
    ref = F.linear(F.layer_norm(x.double(), (K,), gamma.double(), beta.double(), 1e-6), W32.double(), b.double())
    return fold, sep, ref


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_layernorm_fold_vs_separate_layernorm_per_r(dtype):
    """The fold against the LayerNorm it replaces, on rows of r = |mean| / std from 0 to 64, an outlier family and the
    near-constant row.  e = max over the rows of a family of the per-row error max|y - ref| / max|ref| against fp64.

    The fold multiplies the 16-bit copy of the UN-centred row: operand rounding s |x_k| (s = 2^-8 / 2^-11) enters the output as
    s / sqrt(3) sqrt(sum_k x_k^2 w'_k^2) rstd ~ s / sqrt(3) sqrt(1 + r^2) |w'|_2 (rms), where the separate path has s / sqrt(3)
    |w|_2 from its rounded LayerNorm output; both add the rounding of W (s / sqrt(3) |w|_2) and of the output (s).  With the max
    over 2304 columns ~ 4 rms against max|ref| ~ 3.5 rms: e_fold <~ s (1.7 + 0.66 (1 + r)) <= c (1 + r) s with c = 2 for any r,
    and e_fold <= 3 e_sep + 4 s at r <= 1 (the end-to-end tap relation).  The single-pass variance from fp32 records loses
    u (1 + r^2) relative: invisible at r <= 8 (4e-6), a visible share of the error only beyond r ~ 64.

    Measured on MI355X, e_fold / s for bf16 (fp16): r = 0 1.1 (1.3), 1 1.2 (1.4), 2 1.7 (1.4), 4 2.7 (2.5), 8 4.9 (5.0),
    16 10.5 (9.8), 32 19.5 (20.1), 64 41.5 (42.0), outliers 2.2 (2.2); e_sep / s 0.7 .. 2.2 throughout.  The fold tracks
    ~0.6 (1 + r) s, a third of the model's bound, and stays finite; the near-constant row (r = 1000) comes out at 225 s (bf16,
    0.9 relative) and 421 s (fp16, 0.2 relative): there the rounding of the un-centred operand alone exceeds the row's spread."""
    M, K = 1155, 768
    s = STEP[dtype]
    rs = (0.0, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0)
    x, r = rows_with_stats(M, K, r_values=rs, seed=96)
    fold, sep, ref = fold_vs_separate(dtype, x.to(DEV))
    assert torch.isfinite(fold.float()).all() and torch.isfinite(sep.float()).all()
    ef, es = per_row_err(fold, ref).cpu(), per_row_err(sep, ref).cpu()
    nominal = torch.tensor(rs, dtype=torch.float64)[torch.arange(M) % len(rs)]
    nominal[M // 2] = 1000.0
    print(f"\n[fold vs separate {dtype}] per r: e_fold / s, e_sep / s (max over rows)")
    for rv in list(rs) + [1000.0]:
        sel = nominal == rv
        e_f, e_s = float(ef[sel].max()), float(es[sel].max())
        print(f"    r={rv:7.1f}: e_fold {e_f / s:7.2f}  e_sep {e_s / s:5.2f}")
        if rv <= 1.0:
            assert e_f <= 3 * e_s + 4 * s
        if rv in (4.0, 8.0):
            assert e_f <= 2 * (1 + rv) * s
    xo, _ = rows_with_stats(M, K, r_values=(0.0, 0.5, 1.0), outliers=True, near_constant=False, seed=97)
    fold, sep, ref = fold_vs_separate(dtype, xo.to(DEV))
    assert torch.isfinite(fold.float()).all()
    e_f, e_s = float(per_row_err(fold, ref).max()), float(per_row_err(sep, ref).max())
    print(f"    outliers: e_fold {e_f / s:7.2f}  e_sep {e_s / s:5.2f}")
    assert e_f <= 3 * e_s + 4 * s
