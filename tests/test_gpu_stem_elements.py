"""The stem, judged element by element against fp64: the stem convolution (csrc/stem.hip stem_conv_kernel in all four modes,
stem_conv_kernel_wp in the one-plane modes), the stem's GroupNorm + ReLU + max-pool (csrc/norm.hip gn_relu_maxpool_kernel) and
plain GroupNorm (gn_stats_kernel + gn_apply_kernel).

tests/test_gpu_ops.py and tests/test_gpu_stem_upsample_forms.py judge these kernels with one number per tensor, or per
(image, group), on operands of one scale: a truncating store, a wrong value in a small channel or at a dim pixel and a dropped
window tap pass there.  Here every pixel, channel and group has a scale of its own (tests/gpu_util.py stem_operands,
pool_operands), every output is pre-filled with NaN and sits behind guard elements, and every single element is held to the
bars stem_elem_bound / gn_elem_bound, whose fp32 floors tests/test_stem_bound_host.py measures on a CPU -- where it also shows
which mistakes the bars reject.  profiles/stem_elements.md has the figures."""
import functools

import pytest
import torch

from omnidata_amd.engine import DTYPES, load_library
from tests.gpu_util import (GEMM_MODES, GN_ELEM_CASES, POOL_SHAPES, STEM_IO, STEM_SHAPES, Target, assert_elements_inside,
                            debug_flags, gn_elem_bound, gn_params, gn_pool_ref64, gn_ref64, pool_operands, ptr,
                            scaled_gemm_operands, stem_elem_bound, stem_operands, stem_ref64, stream, window_max)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IO_ID = {"fp32": 0, "bf16": 1, "fp16": 2}
ONE_PLANE = ("bf16", "fp16")
TWO_PLANE = ("bf16x3", "fp16x3")
EPS = 1e-5


# ------------------------------------------------------------------------------------------------------------ stem convolution
@functools.lru_cache(maxsize=None)
def stem_ref(case, mode, io):
    _, _, X, Wt = stem_operands(*case)
    y, S = stem_ref64(X, Wt, mode, io)
    return y, stem_elem_bound(mode, y, S)


def run_stem(mode, io, case, flag, misalign=False):
    """fp64 value [B, H/2, W/2, 64] and the raw hi-plane bits of one launch.  misalign: the image starts 8 bytes (fp32) or
    4 bytes (16-bit) behind a 16-byte boundary, where stem_conv_kernel_wp's loads cannot run and the launcher stays on
    stem_conv_kernel; nothing else is moved."""
    B, H, W = case
    x, wp, _, _ = stem_operands(*case)
    n, guard = B * (H // 2) * (W // 2) * 64, (W // 2) * 64
    t = Target(mode, n, guard, 64 * 176)
    try:
        xbuf = torch.zeros(x.numel() + 8, dtype=STEM_IO[io], device=DEV)
        assert xbuf.data_ptr() % 16 == 0
        off = 2 if misalign else 0
        xd = xbuf[off:off + x.numel()]
        xd.copy_(x.float().to(STEM_IO[io]).flatten())
        assert xd.data_ptr() % 16 == (0 if not misalign else (8 if io == "fp32" else 4))
        w = t.put(wp)
        y = t.out()
        with debug_flags(flag):
            rc = load_library().dptx_op_stem_conv_io(DTYPES[mode], ptr(xd), IO_ID[io], ptr(w), ptr(y), B, H, W, stream())
        assert rc == 0
        v = t.value().view(B, H // 2, W // 2, 64)
        return v, y.view(torch.int16).cpu().clone()
    finally:
        t.close()


@pytest.mark.parametrize("mode", ONE_PLANE)
@pytest.mark.parametrize("io", list(STEM_IO))
@pytest.mark.parametrize("case", STEM_SHAPES)
def test_stem_conv_elements_one_plane(mode, io, case):
    """both forms (debug flag 0: stem_conv_kernel_wp; 128: stem_conv_kernel) inside the bar on every element, and equal bit
    for bit on these signed, scaled operands"""
    y, bar = stem_ref(case, mode, io)
    new, new_bits = run_stem(mode, io, case, 0)
    old, old_bits = run_stem(mode, io, case, 128)
    assert_elements_inside(new, y, bar, f"stem {mode} io={io} {case} flag 0")
    assert_elements_inside(old, y, bar, f"stem {mode} io={io} {case} flag 128")
    assert torch.equal(new_bits, old_bits)


@pytest.mark.parametrize("mode", TWO_PLANE)
@pytest.mark.parametrize("io", list(STEM_IO))
@pytest.mark.parametrize("case", STEM_SHAPES)
def test_stem_conv_elements_planes(mode, io, case):
    """stem_conv_kernel<DT, 2>: the kernel splits the image into its hi / lo pair itself; the weight and the output are pairs
    in a PlaneArena"""
    y, bar = stem_ref(case, mode, io)
    got, _ = run_stem(mode, io, case, 0)
    assert_elements_inside(got, y, bar, f"stem {mode} io={io} {case}")


@pytest.mark.parametrize("mode", ONE_PLANE)
@pytest.mark.parametrize("io", list(STEM_IO))
def test_stem_conv_misaligned_image_falls_back_with_the_same_bits(mode, io):
    case = (3, 16, 40)
    _, aligned = run_stem(mode, io, case, 0)
    got, moved = run_stem(mode, io, case, 0, misalign=True)
    y, bar = stem_ref(case, mode, io)
    assert_elements_inside(got, y, bar, f"stem {mode} io={io} {case} misaligned image")
    assert torch.equal(moved, aligned)


# ------------------------------------------------------------------------------------------- GroupNorm (+ ReLU + max-pool)
def gn_scratch(B, HW, C):
    pix = min(max(16384 // C, 16), 256)
    return torch.full((B * ((HW + pix - 1) // pix) * 64,), float("nan"), device=DEV)


def run_groupnorm(mode, x, gamma, beta, R, relu):
    """(fp64 value of dptx_op_groupnorm's output [B, HW, C], fp64 values of the stored input and residual) on the CPU"""
    B, HW, C = x.shape
    t = Target(mode, x.numel(), C, 2 * x.numel())
    try:
        X = t.put(x)
        Rd = None if R is None else t.put(R)
        g, b = gamma.to(DEV), beta.to(DEV)
        Y = t.out()
        rc = load_library().dptx_op_groupnorm(DTYPES[mode], ptr(X), ptr(g), ptr(b), ptr(Rd), ptr(Y), B, HW, C, relu, EPS,
                                              ptr(gn_scratch(B, HW, C)), stream())
        assert rc == 0
        got = t.value().view(B, HW, C)
        stored = (lambda v: None if v is None else (t.arena.value(v) if t.pl == 2 else v.double()).cpu())
        return got, stored(X), stored(Rd)
    finally:
        t.close()


@pytest.mark.parametrize("mode", GEMM_MODES)
@pytest.mark.parametrize("case", POOL_SHAPES)
def test_gn_relu_maxpool_elements(mode, case):
    """(a) every element of dptx_op_gn_relu_maxpool inside gn_elem_bound of gn_pool_ref64; (b) the output IS the 3 x 3 / 2
    max-pool (pad (0, 1) of -inf) of dptx_op_groupnorm(relu=1)'s output on the same input -- rounding and ReLU are monotone
    and the records come from the same kernel, so a one-plane output is the same number; of a pair the value hi + lo is
    compared (near a tie two pairs can carry one value)."""
    B, H, W, C = case
    x = pool_operands(B, H, W, C, seed=C + H)
    gamma, beta = gn_params(C, seed=H)
    t = Target(mode, B * (H // 2) * (W // 2) * C, (W // 2) * C, x.numel())
    try:
        X = t.put(x)
        g, b = gamma.to(DEV), beta.to(DEV)
        Y = t.out()
        rc = load_library().dptx_op_gn_relu_maxpool(DTYPES[mode], ptr(X), ptr(g), ptr(b), ptr(Y), B, H, W, C, EPS,
                                                    ptr(gn_scratch(B, H * W, C)), stream())
        assert rc == 0
        got = t.value().view(B, H // 2, W // 2, C)
        stored = (t.arena.value(X) if t.pl == 2 else X.double()).cpu()
    finally:
        t.close()
    y, T = gn_pool_ref64(stored, gamma, beta, H, W, EPS)
    assert_elements_inside(got, y, gn_elem_bound(mode, y, T), f"gn+relu+maxpool {mode} {case}")
    unpooled, _, _ = run_groupnorm(mode, x, gamma, beta, None, 1)
    pooled = window_max(unpooled.view(B, H, W, C), H, W)
    differ = torch.nonzero(pooled != got)
    assert differ.numel() == 0, (len(differ), differ[:5].tolist())


@pytest.mark.parametrize("mode", GEMM_MODES)
@pytest.mark.parametrize("case", GN_ELEM_CASES)
def test_groupnorm_elements(mode, case):
    """every element of dptx_op_groupnorm inside gn_elem_bound of gn_ref64: cpg = 2, 4, 8, 16, 32 -- every slot path of
    gn_stats_kernel --, ragged last records, with and without residual and ReLU"""
    B, HW, C, relu, res = case
    x = pool_operands(B, HW, 1, C, seed=C + HW)
    gamma, beta = gn_params(C, seed=HW)
    R = scaled_gemm_operands(B * HW, C, 8, seed=C)[3].view(B, HW, C) if res else None
    got, xs, Rs = run_groupnorm(mode, x, gamma, beta, R, relu)
    y, T = gn_ref64(xs, gamma, beta, Rs, relu, EPS)
    assert_elements_inside(got, y, gn_elem_bound(mode, y, T), f"groupnorm {mode} {case}")
