"""fp16x3 and the per-group precision policy ("mixed" dtype, include/dptx.h DPTX_GROUP_*): op-level checks of the fp16
hi/lo split arithmetic (including the property it rests on: gfx950's f16 MFMA does not flush subnormal inputs) and the
end-to-end 1e-3 gate of north_star against the fp32 CPU oracle and the reference-generated golden vectors.
pytest -m gpu."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from omnidata_amd.engine import load_library
from omnidata_amd.model import DPTDepthModel
from tests.gpu_util import PlaneArena, op_gemm, ptr, rel_err, stream
from tests.test_gpu_e2e import oracle_case
from oracle.dpt_oracle import mean_angular_error_deg, ssi_align
from oracle.validate_vs_reference import subsample

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16X3 = 3
TOL = 2e-5  # fp16 planes carry 22 significand bits; what is left is the dropped lo*lo term and the output split


def g(*shape, scale=1.0, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def test_f16_mfma_keeps_subnormal_inputs():
    """lo planes of small values are fp16 subnormals (< 2^-14); the split is only as good as the MFMA's handling of them."""
    M, N, K = 128, 128, 64
    a = torch.full((M, K), 2.0 ** -20, dtype=torch.float16, device=DEV)   # subnormal in fp16
    a[:, 1::2] = 3 * 2.0 ** -24                                             # a few ulps above zero
    w = torch.ones(N, K, dtype=torch.float16, device=DEV)
    c = op_gemm("fp16", a, w, c_fp32=True)
    want = 32 * 2.0 ** -20 + 32 * 3 * 2.0 ** -24
    assert torch.all(c == want), (float(c[0, 0]), want)
    # and as the B operand
    c2 = op_gemm("fp16", w[:M], a[:N], c_fp32=True)
    assert torch.all(c2 == want), (float(c2[0, 0]), want)


@pytest.mark.parametrize("M,N,K", [(1000, 256, 192), (1731, 768, 768), (5000, 32, 1152), (300, 64, 576)])
def test_fp16x3_gemm(M, N, K):
    lib = load_library()
    ar = PlaneArena(M * K + N * K + 2 * M * N + 4096, dtype=torch.float16)
    try:
        # weights of 1/sqrt(K) magnitude: their lo planes are subnormal throughout
        A, W, R = ar.put(g(M, K, seed=1)), ar.put(g(N, K, scale=K ** -0.5, seed=2)), ar.put(g(M, N, seed=3))
        C = ar.empty(M, N)
        bias = torch.randn(N, device=DEV)
        assert lib.dptx_op_gemm(F16X3, ptr(A), ptr(W), ptr(bias), ptr(R), ptr(C), M, N, K, 2, 0, 0, 0, stream()) == 0
        ref = F.gelu(ar.value(A) @ ar.value(W).t() + bias.double()) + ar.value(R)
        assert rel_err(ar.value(C), ref) < TOL
        C32 = torch.empty(M, N, device=DEV)
        assert lib.dptx_op_gemm(F16X3, ptr(A), ptr(W), None, None, ptr(C32), M, N, K, 0, 0, 1, 0, stream()) == 0
        assert rel_err(C32, ar.value(A) @ ar.value(W).t()) < TOL
    finally:
        ar.release()


@pytest.mark.parametrize("B,Hs,Ws,C,relu", [(2, 96, 96, 3, 1), (1, 192, 192, 1, 1), (3, 64, 80, 3, 0), (1, 16, 16, 1, 1)])
def test_fp16x3_fused_head_tail(B, Hs, Ws, C, relu):
    """head_tail_x3_kernel (head.hip): x2 bilinear (align_corners) -> conv3x3 128->32 -> ReLU -> conv1x1 32->C -> ReLU on hi/lo
    fp16 planes with three MFMAs per product, against the chain in fp64 torch on the values the planes hold; the up-sampled
    map is the hi/lo split of the fp32 blend, as upsample2x_kernel<fp16, 2> writes it."""
    lib = load_library()
    ar = PlaneArena(B * Hs * Ws * 128 + 32 * 9 * 128 + B * 4 * Hs * Ws * 128 + 8192, dtype=torch.float16)
    try:
        H0 = ar.put(g(B, Hs, Ws, 128, seed=21))
        W2 = ar.put(g(32, 3, 3, 128, scale=1152 ** -0.5, seed=22))
        b2 = torch.randn(32, device=DEV) * 0.3
        w4 = torch.randn(C, 32, device=DEV) * 0.3
        b4 = torch.randn(C, device=DEV) * 0.2
        y = torch.full((B, C, 2 * Hs, 2 * Ws), float("nan"), device=DEV)
        assert lib.dptx_op_head_tail(F16X3, ptr(H0), ptr(W2), ptr(b2), ptr(w4), ptr(b4), ptr(y), B, Hs, Ws, C, relu, stream()) == 0
        assert torch.isfinite(y).all()
        # this library's own up-sampling of the plane pair (bit-identical window), then fp64
        U = ar.empty(B, 2 * Hs, 2 * Ws, 128)
        assert lib.dptx_op_upsample2x(F16X3, ptr(H0), ptr(U), B, Hs, Ws, 128, stream()) == 0
        h = F.relu(F.conv2d(ar.value(U).permute(0, 3, 1, 2), ar.value(W2).permute(0, 3, 1, 2), b2.double(), padding=1))
        ref = F.conv2d(h, w4.double().view(C, 32, 1, 1), b4.double())
        if relu:
            ref = F.relu(ref)
        err = rel_err(y, ref)
        print(f"\n[fp16x3 fused head tail B={B} {Hs}x{Ws} C={C}] rel err vs fp64 {err:.2e}")
        # 1.5 x TOL: the measure is max |err| / max |ref| over ONE output channel when C = 1, i.e. it scales with the draw of the
        # 32 head weights (1.5e-5 ... 2.1e-5 over the round's full runs); the other op tests of this file use TOL itself
        assert err < 1.5 * TOL
        # and within fp32 interpolation rounding of torch's own bilinear on the exact values
        up = F.interpolate(ar.value(H0).permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
        h = F.relu(F.conv2d(up, ar.value(W2).permute(0, 3, 1, 2), b2.double(), padding=1))
        ref2 = F.conv2d(h, w4.double().view(C, 32, 1, 1), b4.double())
        if relu:
            ref2 = F.relu(ref2)
        assert rel_err(y, ref2) < 2 * TOL
    finally:
        ar.release()


@pytest.mark.parametrize("case", [(2, 24, 256, 256, 3, 1, 1, 24, 1, 1), (3, 48, 128, 128, 3, 2, 0, 24, 0, 0)])
def test_fp16x3_conv(case):
    from tests.test_gpu_ops import conv_ref
    lib = load_library()
    B, H, Cin, Cout, k, stride, pad, Ho, a_relu, act = case
    ar = PlaneArena(B * H * H * Cin + Cout * k * k * Cin + 2 * B * Ho * Ho * Cout + 4096, dtype=torch.float16)
    try:
        X, Wt = ar.put(g(B, H, H, Cin, seed=4)), ar.put(g(Cout, k, k, Cin, scale=(k * k * Cin) ** -0.5, seed=5))
        R, Y = ar.put(g(B, Ho, Ho, Cout, seed=6)), ar.empty(B, Ho, Ho, Cout)
        bias = torch.randn(Cout, device=DEV) * 0.1
        assert lib.dptx_op_conv(F16X3, ptr(X), ptr(Wt), ptr(bias), ptr(R), ptr(Y), B, H, H, Cin, Cout, k, stride, pad, pad, Ho, Ho,
                                a_relu, act, stream()) == 0
        ref = conv_ref(ar.value(X), ar.value(Wt), bias, stride, pad, pad, Ho, Ho, a_relu).double()
        if act == 1:
            ref = F.relu(ref)
        ref = ref + ar.value(R)
        assert rel_err(ar.value(Y), ref) < TOL
    finally:
        ar.release()


def test_fp16x3_norms_attention():
    lib = load_library()
    B, HW, C, S, H = 2, 2304, 128, 577, 12
    ar = PlaneArena(3 * B * HW * C + B * S * 4 * H * 64 + 4096, dtype=torch.float16)
    try:
        X, R, Y = ar.put(g(B, HW, C, seed=8) * 2 + 0.5), ar.put(g(B, HW, C, seed=9)), ar.empty(B, HW, C)
        gm, bt = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
        scratch = torch.empty(B * 144 * 64, device=DEV)
        assert lib.dptx_op_groupnorm(F16X3, ptr(X), ptr(gm), ptr(bt), ptr(R), ptr(Y), B, HW, C, 1, 1e-5, ptr(scratch), stream()) == 0
        ref = F.relu(F.group_norm(ar.value(X).permute(0, 2, 1), 32, gm.double(), bt.double(), 1e-5).permute(0, 2, 1) + ar.value(R))
        assert rel_err(ar.value(Y), ref) < TOL
        q0 = g(B, S, 3, H, 64, seed=7)
        qkv = ar.put(q0.reshape(B * S, 3 * H * 64))
        out = ar.empty(B * S, H * 64)
        assert lib.dptx_op_attention(F16X3, ptr(qkv), ptr(out), B, S, H, stream()) == 0
        q3 = ar.value(qkv).view(B, S, 3, H, 64)
        q, k, v = [t.permute(0, 2, 1, 3) for t in q3.unbind(2)]
        ref = (((q @ k.transpose(-1, -2)) * 0.125).softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B * S, H * 64)
        assert rel_err(ar.value(out), ref) < 2 * TOL
    finally:
        ar.release()


def test_fp16x3_norms_per_row_and_group_statistics():
    """the fp16 hi / lo planes of tests/test_gpu_x3.py's plane_norms_per_stats (the stem's GroupNorm + ReLU + MaxPool2dSame runs
    in this mode under the default `mixed` policy)"""
    from tests.test_gpu_x3 import plane_norms_per_stats
    plane_norms_per_stats(F16X3, torch.float16, TOL)


# (dtype, x3_groups, max-abs bar): the first two are parity modes (north_star 1e-3); the third shows what the policy that
# only protects the ResNet stages buys (emulated floor 1.5e-3 on these weights, oracle/precision_policy.py)
POLICIES = [("mixed", 0, 1e-3), ("fp16x3", 0, 1e-3), ("mixed", "resnet", 2.5e-3)]


@pytest.mark.parametrize("dtype,groups,bar", POLICIES, ids=["mixed-default", "fp16x3", "mixed-resnet"])
@pytest.mark.parametrize("task,C,seed,B", [("normal", 3, 0, 1), ("depth", 1, 0, 1), ("normal", 3, 1, 2)])
def test_policy_end_to_end(task, C, seed, B, dtype, groups, bar):
    """north_star: outputs within 1e-3 abs of the PyTorch-CPU fp32 forward (normal map / scale-invariant depth)."""
    sd, x, ref, _ = oracle_case(task, C, seed, B)
    model = DPTDepthModel(num_channels=C, dtype=dtype, max_batch=B, x3_groups=groups)
    model.load_state_dict(sd)
    model.to(DEV)
    y = model(x.to(DEV)).cpu()
    d = (y - ref).abs()
    print(f"\n[{task} seed={seed} B={B} {dtype}/{groups}] max|d|={d.max():.3e} rms={d.pow(2).mean().sqrt():.3e}")
    assert y.shape == ref.shape and torch.isfinite(y).all()
    assert d.max().item() < bar
    if task == "normal":
        assert mean_angular_error_deg(y.clamp(0, 1), ref.clamp(0, 1)) < 0.08 * bar / 1e-3
    else:
        assert (ssi_align(y, ref) - ref).abs().max().item() < bar


def test_mixed_stage_taps():
    """Stage taps of the default policy: 3-MFMA groups sit at the fp32 level, the ViT blocks at the fp16 level."""
    sd, x, ref, otaps = oracle_case("normal", 3, 0, 1)
    model = DPTDepthModel(num_channels=3, dtype="mixed", max_batch=1)
    model.load_state_dict(sd)
    model.to(DEV)
    eng = model._get_engine(torch.device(DEV))
    eng.enable_taps(True)
    model(x.to(DEV))
    rel = {}
    for n in ["stem", "s0", "s1", "s2", "tok0", "blk0", "blk8", "blk11", "l3", "l4", "l1_rn", "l4_rn", "p4", "p1", "h0", "h1"]:
        got, want = eng.tap(n), otaps[n]
        rel[n] = ((got - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt()).item()
        print(f"    tap {n:6s} rms-rel err {rel[n]:.3e}")
    assert max(rel[n] for n in ("stem", "s0", "s1", "s2", "tok0")) < 5e-5   # 3-MFMA layers upstream of the ViT blocks
    assert rel["l1_rn"] < 5e-4   # layer1_rn is single-pass in the default per-layer table: one fp16 operand rounding
    assert max(rel.values()) < 2e-3


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "dpt_*.npz"))),
                         ids=lambda p: os.path.basename(p))
def test_mixed_vs_reference_golden(path):
    gd = np.load(path)
    task, C, seed, B = str(gd["task"]), int(gd["num_channels"]), int(gd["seed"]), int(gd["batch"])
    sd, x, _, _ = oracle_case(task, C, seed, B)
    model = DPTDepthModel(num_channels=C, dtype="mixed", max_batch=B)
    model.load_state_dict(sd)
    model.to(DEV)
    y = model(x.to(DEV)).cpu()
    d = np.abs(subsample(y) - gd["out_sub"])
    print(f"\n[{os.path.basename(path)} mixed] vs reference golden: max|d|={d.max():.3e}")
    assert d.max() < 1e-3


def test_default_model_is_the_parity_mode():
    """The drop-in surface defaults to the mode that matches the reference: a default-constructed DPTDepthModel (what
    hubconf.py and demo.py build) is 'mixed' and meets north_star's 1e-3 against the fp32 oracle."""
    sd, x, ref, _ = oracle_case("normal", 3, 0, 1)
    model = DPTDepthModel(num_channels=3, max_batch=1)
    assert model.engine_dtype == "mixed"
    model.load_state_dict(sd)
    model.to(DEV)
    d = (model(x.to(DEV)).cpu() - ref).abs()
    assert d.max().item() < 1e-3


def test_mixed_b32_vs_oracle_and_batch_invariance():
    """The 1e-3 gate at the BENCHMARK batch (32 images through the two-plane arena, the 8-wave 3-MFMA tiles and the
    two-stream split), against the fp32 oracle on all 32 images; plus bit-level determinism and batch invariance of the
    parity mode: image i of the batch equals the same image run alone, and a second run returns the same bits."""
    from omnidata_amd.weights import random_state_dict, synthetic_input
    from oracle.dpt_oracle import dpt_forward, oracle_threads
    sd = random_state_dict(0, 3)
    x = synthetic_input(7, 32, "normal")
    model = DPTDepthModel(num_channels=3, dtype="mixed", max_batch=32)
    model.load_state_dict(sd)
    model.to(DEV)
    y1 = model(x.to(DEV)).clone()
    y2 = model(x.to(DEV))
    assert torch.equal(y1, y2)
    for i in (0, 15, 16, 31):  # first / last image of both half-batch regions
        assert torch.equal(model(x[i:i + 1].to(DEV))[0], y1[i]), i
    oracle_threads()
    worst, sq, n = 0.0, 0.0, 0
    for i in range(0, 32, 4):
        ref = dpt_forward(sd, x[i:i + 4])
        d = (y1[i:i + 4].cpu() - ref).abs()
        worst = max(worst, d.max().item())
        sq += d.pow(2).sum().item()
        n += d.numel()
    print(f"\n[mixed B=32] max|d|={worst:.3e} rms={(sq / n) ** 0.5:.3e} over {n} outputs")
    assert worst < 1e-3


def test_single_pass_conv_with_two_plane_epilogue():
    """Per-layer policy building block (gemm_impl.h PLE): an fp16 convolution that spends ONE MFMA per product on the hi planes
    but reads its residual as a hi/lo pair and writes a hi/lo result -- against fp64 of exactly that (hi(X) * hi(W) + R), and
    with c_hi_only the lo plane of the output is left alone."""
    lib = load_library()
    B, H, C = 2, 24, 256
    ar = PlaneArena(B * H * H * C * 3 + C * 9 * C + 8192, dtype=torch.float16)
    try:
        X = ar.put(g(B, H, H, C, seed=21))
        Wt = ar.put(g(C, 3, 3, C, scale=(9 * C) ** -0.5, seed=22))
        R = ar.put(g(B, H, H, C, seed=23))
        bias = torch.randn(C, device=DEV) * 0.1
        Y = ar.empty(B, H, H, C)
        rc = lib.dptx_op_conv_planes(1, ptr(X), ptr(Wt), ptr(bias), ptr(R), ptr(Y), B, H, H, C, C, 3, 1, 1, 1, H, H, 1, 0, 1, 0, 0, stream())
        assert rc == 0
        ref = F.conv2d(F.relu(X.double()).permute(0, 3, 1, 2), Wt.double().permute(0, 3, 1, 2), bias.double(), padding=1)
        ref = ref.permute(0, 2, 3, 1) + ar.value(R)
        assert rel_err(ar.value(Y), ref) < 2 * TOL          # result carries 22 bits although the product used 11-bit operands
        assert rel_err(Y.double(), ref) < 8e-4               # and its hi plane is the fp16 rounding of it
        # c_hi_only: the lo plane is not written
        o = (Y.data_ptr() - ar.buf.data_ptr()) // 2
        ar.buf[1, o:o + Y.numel()] = 7.0
        rc = lib.dptx_op_conv_planes(1, ptr(X), ptr(Wt), ptr(bias), ptr(R), ptr(Y), B, H, H, C, C, 3, 1, 1, 1, H, H, 1, 0, 1, 1, 0, stream())
        assert rc == 0 and bool((ar.buf[1, o:o + Y.numel()] == 7.0).all())
        # r1_hi_only: the residual's lo plane is ignored
        ar.buf[1, o:o + Y.numel()] = 0.0
        rc = lib.dptx_op_conv_planes(1, ptr(X), ptr(Wt), ptr(bias), ptr(R), ptr(Y), B, H, H, C, C, 3, 1, 1, 1, H, H, 1, 0, 1, 0, 1, stream())
        ref_hi = ref - ar.value(R) + R.double()
        assert rc == 0 and rel_err(ar.value(Y), ref_hi) < 2 * TOL
    finally:
        ar.release()


@pytest.mark.parametrize("epi2", [0, 2])
def test_two_plane_ping_pong_kernel_equals_the_lockstep_kernel(epi2):
    """gemm_pp2_kernel (round 4: ping-pong schedule of the two wave groups in the two-plane 128x128 tile) runs the MFMAs of
    every accumulator in the same order as the lockstep gemm_glds_kernel: bit-identical planes, 3- and 2-MFMA form, on a shape
    with padding taps, a ragged last tile (M % 128 != 0) and a residual."""
    lib = load_library()
    B, H, W, C, N = 3, 96, 90, 256, 256
    ar = PlaneArena(B * H * W * (C + 3 * N) + N * 9 * C + 8192, dtype=torch.float16)
    try:
        X = ar.put(g(B, H, W, C, seed=41))
        Wt = ar.put(g(N, 3, 3, C, scale=(9 * C) ** -0.5, seed=42))
        R = ar.put(g(B, H, W, N, seed=43))
        bias = torch.randn(N, device=DEV) * 0.1
        outs = []
        for flags in (0, 4):
            assert lib.dptx_debug_set_gemm_flags(flags) == 0
            Y = ar.empty(B, H, W, N)
            rc = lib.dptx_op_conv_planes(F16X3, ptr(X), ptr(Wt), ptr(bias), ptr(R), ptr(Y), B, H, W, C, N, 3, 1, 1, 1, H, W, 0, 1, epi2, 0, 0, stream())
            assert rc == 0
            outs.append(ar.value(Y).clone())
        lib.dptx_debug_set_gemm_flags(0)
        assert torch.equal(outs[0], outs[1])
        ref = F.relu(F.conv2d(ar.value(X).permute(0, 3, 1, 2) if epi2 == 0 else X.double().permute(0, 3, 1, 2),
                              ar.value(Wt).permute(0, 3, 1, 2), bias.double(), padding=1)).permute(0, 2, 3, 1) + ar.value(R)
        assert rel_err(outs[0], ref) < TOL
    finally:
        lib.dptx_debug_set_gemm_flags(0)
        ar.release()


@pytest.mark.parametrize("B,H,a_relu,N", [(3, 96, 0, 128), (3, 96, 1, 256), (2, 48, 1, 256), (2, 48, 0, 64)])  # 128x128 (8 waves) x2, 64x64 x2
def test_two_mfma_conv_rounds_only_its_input(B, H, a_relu, N):
    """Per-layer precision 2 (gemm_impl.h XT == 2, GemmParams::a_hi_only): both planes of the weights, the hi plane of the
    activations -- against fp64 of exactly that (fp16(X) * (W_hi + W_lo) + R); the lo plane of X is NaN: it is not read."""
    lib = load_library()
    C = 256
    ar = PlaneArena(B * H * H * (C + 3 * N) + N * 9 * C + 8192, dtype=torch.float16)
    try:
        X = ar.put(g(B, H, H, C, seed=31))
        Wt = ar.put(g(N, 3, 3, C, scale=(9 * C) ** -0.5, seed=32))
        R = ar.put(g(B, H, H, N, seed=33))
        bias = torch.randn(N, device=DEV) * 0.1
        Y = ar.empty(B, H, H, N)
        o = (X.data_ptr() - ar.buf.data_ptr()) // 2
        ar.buf[1, o:o + X.numel()] = float("nan")
        rc = lib.dptx_op_conv_planes(F16X3, ptr(X), ptr(Wt), ptr(bias), ptr(R), ptr(Y), B, H, H, C, N, 3, 1, 1, 1, H, H, a_relu, 0, 2, 0, 0, stream())
        assert rc == 0
        xin = F.relu(X.double()) if a_relu else X.double()
        ref = F.conv2d(xin.permute(0, 3, 1, 2), ar.value(Wt).permute(0, 3, 1, 2), bias.double(), padding=1).permute(0, 2, 3, 1) + ar.value(R)
        got = ar.value(Y)
        assert torch.isfinite(got).all()
        assert rel_err(got, ref) < TOL
        # the 3-MFMA form on the same operands (lo plane of X zero) gives the same values up to the accumulation order
        ar.buf[1, o:o + X.numel()] = 0.0
        Y3 = ar.empty(B, H, H, N)
        rc = lib.dptx_op_conv_planes(F16X3, ptr(X), ptr(Wt), ptr(bias), ptr(R), ptr(Y3), B, H, H, C, N, 3, 1, 1, 1, H, H, a_relu, 0, 0, 0, 0, stream())
        assert rc == 0 and rel_err(ar.value(Y3), ref) < TOL
    finally:
        ar.release()


def test_two_mfma_head_conv_sits_between_one_and_three():
    """dptx_set_layer_precision(..., 2) on scratch.output_conv.0 (the measured option of round 4, not the default): (a) 3 MFMAs
    on that layer is at least as close to the oracle, 1 MFMA is further away -- 2 sits between and still meets 1e-3; (b) with
    2 MFMAs path_1 carries no lo plane: a forward over an arena full of NaN gives the same bits."""
    from omnidata_amd.engine import Engine
    sd, x, ref, _ = oracle_case("normal", 3, 0, 1)
    xd = x.to(DEV)
    rms = {}
    for m in (1, 2, 3):
        e = Engine(num_channels=3, max_batch=1, dtype="mixed", device_id=0)
        e.load_state_dict(sd)
        if m != 3:   # (3 = the default table's assignment: the layer follows its group)
            e.set_layer_precision("scratch.output_conv.0.weight", m)
        y = e.forward(xd).cpu()
        if m == 2:
            e.arena_fill(0xFF)
            assert torch.equal(e.forward(xd).cpu(), y)
        d = (y - ref).abs()
        rms[m] = (d.pow(2).mean().sqrt().item(), d.max().item())
        e.close()
    print(f"\n[mixed, output_conv.0 with 1 / 2 / 3 MFMAs] rms {rms[1][0]:.3e} / {rms[2][0]:.3e} / {rms[3][0]:.3e}, "
          f"max {rms[1][1]:.3e} / {rms[2][1]:.3e} / {rms[3][1]:.3e}")
    assert rms[3][0] <= rms[2][0] * 1.05 and rms[2][0] <= rms[1][0] * 1.05
    assert rms[2][1] < 1e-3


DECODER_CONVS = (["scratch.layer%d_rn.weight" % i for i in (1, 2, 3, 4)] +
                 ["scratch.refinenet%d.resConfUnit%d.conv%d.weight" % (i, u, c) for i in (1, 2, 3, 4) for u in (1, 2) for c in (1, 2)
                  if not (i == 4 and u == 1)] +
                 ["scratch.refinenet%d.out_conv.weight" % i for i in (1, 2, 3, 4)] +
                 ["scratch.output_conv.0.weight", "scratch.output_conv.2.weight"])


def test_per_layer_policy_api_and_group_policy_flag():
    """dptx_set_layer_precision / DPTX_FLAG_GROUP_POLICY: (a) every decoder convolution switched to one MFMA through the
    per-layer API gives the same bits as the group-level policy that leaves the decoder groups single-pass; (b) the group-level
    policy of round 2 (flag 2) still meets 1e-3 and is at least as close to the oracle as the default per-layer table."""
    from omnidata_amd.engine import Engine
    sd, x, ref, _ = oracle_case("normal", 3, 0, 1)
    xd = x.to(DEV)
    a = Engine(num_channels=3, max_batch=1, dtype="mixed", device_id=0, x3_groups="resnet+embed+reassemble")
    a.load_state_dict(sd)
    ya = a.forward(xd).cpu()
    a.close()
    b = Engine(num_channels=3, max_batch=1, dtype="mixed", device_id=0)
    b.load_state_dict(sd)
    for k in DECODER_CONVS:
        b.set_layer_precision(k, 1)
    yb = b.forward(xd).cpu()
    with pytest.raises(RuntimeError):
        b.set_layer_precision("pretrained.model.blocks.0.attn.qkv.weight", 3)   # not a decoder convolution
    b.close()
    assert torch.equal(ya, yb)
    errs = {}
    for name, flags in (("per-layer default", 0), ("group-level (round 2)", 2)):
        e = Engine(num_channels=3, max_batch=1, dtype="mixed", device_id=0, flags=flags)
        e.load_state_dict(sd)
        d = (e.forward(xd).cpu() - ref).abs()
        errs[name] = (d.max().item(), d.pow(2).mean().sqrt().item())
        e.close()
        print(f"\n[mixed, {name}] max|d|={errs[name][0]:.3e} rms={errs[name][1]:.3e}")
    assert errs["per-layer default"][0] < 1e-3 and errs["group-level (round 2)"][0] < 1e-3
    assert errs["group-level (round 2)"][1] < 1.2 * errs["per-layer default"][1]


def test_default_model_leaves_fp16_planes_when_they_overflow():
    """fp16 hi planes overflow at 65504 and nothing in the forward clamps.  The decoder is re-parameterised
    to compute the SAME function with 1e8 x larger internal activations (ReLU is positively homogeneous: layerN_rn weights
    and every refinenet bias x 1e8, first head conv weight / 1e8; two fp16 planes still represent 1e5): the default model must notice the non-finite result of
    its first image's activations, switch to bf16 planes (fp32's range) and still match the fp32 oracle."""
    import warnings
    sd, x, ref, _ = oracle_case("normal", 3, 0, 1)
    big = {k: v.clone() for k, v in sd.items()}
    for k in big:
        if k.startswith("scratch.layer") and k.endswith("_rn.weight"):
            big[k] *= 1.0e8
        if k.startswith("scratch.refinenet") and k.endswith(".bias"):
            big[k] *= 1.0e8
    big["scratch.output_conv.0.weight"] /= 1.0e8
    model = DPTDepthModel(num_channels=3, max_batch=1).eval()
    model.load_state_dict(big)
    model = model.to(DEV)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        y = model(x.to(DEV)).float().cpu()
    assert model.engine_dtype == "bf16x3" and any("fp16 range" in str(i.message) for i in w)
    assert torch.isfinite(y).all()
    d = (y - ref).abs().max().item()
    print(f"    default model on 1e8x activations: fell back to bf16x3, max|d| vs oracle {d:.2e}")
    assert d < 1e-3
    # a model that is told to keep its dtype keeps it -- and is wrong (the decoder's ReLUs turn the NaNs back into zeros:
    # the RESULT may well be finite, which is why the check reads the stage taps)
    keep = DPTDepthModel(num_channels=3, max_batch=1, overflow_fallback=False).eval()
    keep.load_state_dict(big)
    y2 = keep.to(DEV)(x.to(DEV)).float().cpu()
    assert keep.engine_dtype == "mixed"
    assert not torch.isfinite(y2).all() or (y2 - ref).abs().max().item() > 1e-2
