"""What the bounds of tests/test_gpu_unet_gemm_elements.py are worth, on a CPU.

(a) The fp32 floor of gemm_elem_bound was measured for K <= 6912; the UNet's GEMM-path convolutions reach K = 9216 (the 1024 ->
    1024 layers) and K = 13824 (up_blocks.5.conv1) at M as small as 1.  The quantity of test_gemm_bound_host.measured_floor --
    the largest |y32 - y| / S of A W^T + bias + R in plain fp32 -- at those K must not exceed the committed constant, so that
    constant and its factor apply to the UNet's layers unchanged.  (These shapes stay out of GEMM_HOST_SHAPES: the mutant
    tests loop over that.)
(b) The head's bound (gpu_util.unet_head_ref64, derived, no measured constant): the kernel's arithmetic in fp32 in the kernel's
    order lies inside it on the inputs of the GPU test, and each of three mistakes such a kernel can make leaves it in more
    than 1 % of the elements.
`python -m tests.test_unet_bound_host` prints the figures profiles/unet_elements.md quotes."""
import pytest
import torch

from tests.gpu_util import (GEMM_F32_FLOOR_MEASURED, UNET_HEAD_HW, UNET_HEAD_OC, gemm_ref64, unet_head_model32,
                            unet_head_operands, unet_head_ref64)
from tests.test_gemm_bound_host import gemm_case

UNET_FLOOR_SHAPES = ((200, 64, 9216), (200, 64, 13824), (3, 128, 9216), (1, 64, 13824))
HEAD_MUTANTS = ("round16", "beta_shift", "late_relu")
HEAD_B = 3


def unet_floor():
    out = {}
    for mode in ("bf16", "fp16"):
        for M, N, K in UNET_FLOOR_SHAPES:
            acc, bias, Av, Wv, Rv, _ = gemm_case(M, N, K, mode)
            y32 = acc + bias + Rv.float()
            y, S = gemm_ref64(Av, Wv, bias, Rv)
            out[(mode, M, N, K)] = float(((y32.double() - y).abs() / S).max())
    return out


def test_fp32_floor_holds_at_the_unets_k():
    for key, v in unet_floor().items():
        print(f"\n[unet floor] {key}: {v:.3e}")
        assert v <= GEMM_F32_FLOOR_MEASURED, (key, v)


def head_outside(dtype, HW, OC, mutant=None):
    """(worst |err| / bound, share of elements outside the bound) of the fp32 model of one case of the GPU test"""
    ops = unet_head_operands(dtype, HEAD_B, HW, OC, seed=HW + OC)
    y, bound = unet_head_ref64(*ops)
    err = (unet_head_model32(*ops, mutant=mutant, dtype=dtype).double() - y).abs()
    return float((err / bound).max()), float((~(err <= bound)).double().mean())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_head_model_is_inside_the_bound(dtype):
    for HW in UNET_HEAD_HW:
        for OC in UNET_HEAD_OC:
            worst, share = head_outside(dtype, HW, OC)
            print(f"\n[unet head model {dtype} HW={HW} OC={OC}] worst |err| / bound {worst:.3f}")
            assert share == 0.0, (dtype, HW, OC, worst)


@pytest.mark.parametrize("mutant", HEAD_MUTANTS)
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_head_mutants_leave_the_bound(dtype, mutant):
    for HW in UNET_HEAD_HW[1:]:            # HW = 1 has 3 * OC elements: no share of 1 % to speak of
        for OC in UNET_HEAD_OC:
            worst, share = head_outside(dtype, HW, OC, mutant)
            print(f"\n[unet head {mutant} {dtype} HW={HW} OC={OC}] share of elements outside the bound {share:.3f}")
            assert share > 0.01, (mutant, dtype, HW, OC, share)


if __name__ == "__main__":
    for key, v in unet_floor().items():
        print("floor", key, f"{v:.3e}")
    for dtype in ("bf16", "fp16"):
        for HW in UNET_HEAD_HW:
            for OC in UNET_HEAD_OC:
                print(f"head model {dtype} HW={HW} OC={OC}: worst |err| / bound {head_outside(dtype, HW, OC)[0]:.3f}; outside: " +
                      ", ".join(f"{m} {head_outside(dtype, HW, OC, m)[1]:.3f}" for m in HEAD_MUTANTS))
