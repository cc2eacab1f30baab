"""What tests/gpu_util.gemm_elem_bound is worth, on a CPU: the tests of tests/test_gpu_gemm_elements.py's tests.

The model is the arithmetic of the implicit-GEMM kernels' epilogue (csrc/gemm_impl.h) in plain torch: operands rounded to one
16-bit plane or split into a hi / lo pair (three products, the lo * lo one dropped), fp32 accumulation, + bias, activation,
+ residual, and ONE rounding of the fp32 value to the stored type (hi = rn(v), lo = rn(v - hi) for a pair).  What it does not
model is the order of the fp32 additions inside an MFMA: that is the fp32 floor of the bound.

Three things are asserted:
  (a) the committed floor constant is what the CPU measures (at least the measurement, at most twice it);
  (b) the honest model violates the bound nowhere, GELU and residual cases included: a correct kernel can meet it;
  (c) every mutant -- the model with one of the mistakes such a kernel can make -- leaves the bound on at least one case: the
      bound is not slack, and the operands are such that the mistake shows.
`python -m tests.test_gemm_bound_host` prints the survey profiles/gemm_elements.md quotes."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import (GEMM_F32_FLOOR_MEASURED, GEMM_HOST_SHAPES, GEMM_MODES, GEMM_PLANES, conv_ref64, elements_outside,
                            gemm_elem_bound, gemm_operand_planes, gemm_ref64, scaled_conv_operands, scaled_gemm_operands)

# (B, H, W, Cin, Cout, k, stride, pad_t, pad_l, Ho, Wo): the first three convolution cases of the GPU file
CONV_CASES = ((3, 10, 14, 64, 64, 3, 1, 1, 1, 10, 14), (2, 9, 14, 128, 128, 3, 2, 1, 0, 5, 7), (2, 14, 9, 128, 128, 3, 2, 0, 1, 7, 5))
EPILOGUES = ("plain", "relu", "gelu", "res", "res32")     # bias everywhere but in "plain"; res32: fp32 R and fp32 C


def store(v, mode, mutant=None):
    """the VALUE (fp64) of the fp32 tensor v as the epilogue stores it: the nearest 16-bit number, or a hi + lo pair."""
    dt, pl = GEMM_PLANES[mode]
    hi = v.to(dt)
    if mutant == "truncate":      # toward zero: one step back wherever rounding went away from zero
        step = torch.where(hi.float().abs() > v.abs(), 1, 0).to(torch.int16)
        hi = (hi.view(torch.int16) - step).view(dt)
    if pl == 1 or mutant == "lozero":
        return hi.double()
    return hi.double() + (v - hi.float()).to(dt).double()


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K, mode):
    """the planes of one GEMM case, its fp32 accumulators (as the kernel forms them) and the fp64 pieces of the reference"""
    A, W, bias, R = scaled_gemm_operands(M, N, K)
    (ah, al), (wh, wl), (rh, rl) = (gemm_operand_planes(t, mode) for t in (A, W, R))
    if al is None:
        acc = ah.float() @ wh.float().t()
        Av, Wv, Rv = ah.double(), wh.double(), rh.double()
    else:
        acc = ah.float() @ wl.float().t() + al.float() @ wh.float().t() + ah.float() @ wh.float().t()
        Av, Wv, Rv = ah.double() + al.double(), wh.double() + wl.double(), rh.double() + rl.double()
    return acc, bias.float(), Av, Wv, Rv, R.float()


def gemm_model(M, N, K, mode, epi, mutant=None):
    """(stored value, y, S, bound) of one case of the model; mutant: truncate / lozero (store), late_residual (the residual is
    added to the ROUNDED value and the sum rounded again), rowshift (row m holds the result of row m - 1)."""
    acc, bias, Av, Wv, Rv, R32 = gemm_case(M, N, K, mode)
    act = {"relu": 1, "gelu": 2}.get(epi, 0)
    v = acc if epi == "plain" else acc + bias
    v = F.relu(v) if act == 1 else F.gelu(v) if act == 2 else v
    res = Rv.float() if epi == "res" else R32 if epi == "res32" else None
    if res is not None:
        v = store(v, mode).float() + res if mutant == "late_residual" else v + res
    out = v.double() if epi == "res32" else store(v, mode, mutant)
    if mutant == "rowshift":
        out = out.roll(1, 0)
    y, S = gemm_ref64(Av, Wv, None if epi == "plain" else bias, None if res is None else res.double(), act)
    return out, y, S, gemm_elem_bound(mode, y, S, act, c_fp32=(epi == "res32"))


def conv_model(case, mode, res=False, mutant=None):
    """(stored value, y, S, bound) of one convolution case; mutant: padswap (pad_t and pad_l exchanged), wrap (the tap left of
    column 0 reads the element in front of it in memory -- the last pixel of the row above -- instead of zero)."""
    B, H, W, Cin, Cout, k, stride, pad_t, pad_l, Ho, Wo = case
    X, Wt, bias, R = scaled_conv_operands(B, H, W, Cin, Cout, k, 0, Ho, Wo)
    (xh, xl), (wh, wl), (rh, rl) = (gemm_operand_planes(t, mode) for t in (X, Wt, R))
    two = xl is not None
    Xv, Wv, Rv = (xh.double() + xl.double(), wh.double() + wl.double(), rh.double() + rl.double()) if two else (xh.double(), wh.double(), rh.double())
    pt, pl_ = (pad_l, pad_t) if mutant == "padswap" else (pad_t, pad_l)

    def conv32(x, w):
        x = x.float().permute(0, 3, 1, 2)
        pb, pr = max((Ho - 1) * stride + k - H - pt, 0), max((Wo - 1) * stride + k - W - pl_, 0)
        xp = F.pad(x, [pl_, pr, pt, pb])
        if mutant == "wrap" and pl_ > 0:
            xp[:, :, pt + 1:pt + H, pl_ - 1] = x[:, :, :H - 1, W - 1]
        return F.conv2d(xp, w.float().permute(0, 3, 1, 2), None, stride)[:, :, :Ho, :Wo].permute(0, 2, 3, 1)

    acc = conv32(xh, wl) + conv32(xl, wh) + conv32(xh, wh) if two else conv32(xh, wh)
    v = acc + bias.float()
    if res:
        v = v + Rv.float()
    y, S = conv_ref64(Xv, Wv, bias.float(), Rv if res else None, stride, pad_t, pad_l, Ho, Wo)
    return store(v, mode), y, S, gemm_elem_bound(mode, y, S, 0)


def measured_floor():
    """largest |y32 - y| / S of A W^T + bias + R in plain fp32 over GEMM_HOST_SHAPES x the two types, per case"""
    out = {}
    for mode in ("bf16", "fp16"):
        for M, N, K in GEMM_HOST_SHAPES:
            acc, bias, Av, Wv, Rv, _ = gemm_case(M, N, K, mode)
            y32 = acc + bias + Rv.float()
            y, S = gemm_ref64(Av, Wv, bias, Rv)
            out[(mode, M, N, K)] = float(((y32.double() - y).abs() / S).max())
    return out


def test_fp32_floor_is_what_the_bound_uses():
    worst = max(measured_floor().values())
    assert worst <= GEMM_F32_FLOOR_MEASURED <= 2.0 * worst, worst


def test_conv_ref64_is_conv2d():
    """conv_ref64 (one matrix product per tap) against F.conv2d in fp64 with the explicit bottom / right padding"""
    for B, H, W, Cin, Cout, k, stride, pad_t, pad_l, Ho, Wo in CONV_CASES:
        X, Wt, bias, _ = scaled_conv_operands(B, H, W, Cin, Cout, k, 0, Ho, Wo)
        for a_relu in (0, 1):
            y, S = conv_ref64(X, Wt, bias, None, stride, pad_t, pad_l, Ho, Wo, a_relu)
            x = (F.relu(X) if a_relu else X).permute(0, 3, 1, 2)
            xp = F.pad(x, [pad_l, max((Wo - 1) * stride + k - W - pad_l, 0), pad_t, max((Ho - 1) * stride + k - H - pad_t, 0)])
            want = F.conv2d(xp, Wt.permute(0, 3, 1, 2), bias, stride).permute(0, 2, 3, 1)
            wantS = F.conv2d(xp.abs(), Wt.abs().permute(0, 3, 1, 2), bias.abs(), stride).permute(0, 2, 3, 1)
            assert want.shape == y.shape == (B, Ho, Wo, Cout)
            assert ((y - want).abs() <= 1e-13 * S).all() and ((S - wantS).abs() <= 1e-13 * S).all()


def test_operand_scales():
    """adjacent rows and adjacent columns differ in scale by 2^2 at least; values inside fp16"""
    A, W, bias, R = scaled_gemm_operands(300, 64, 64)
    ra, rw = A.abs().amax(1).log2(), W.abs().amax(1).log2()
    assert ((ra[1:] - ra[:-1]).abs() > 3.0).all() and ((rw[1:] - rw[:-1]).abs() > 0.5).all()
    assert (((7 * torch.arange(300)) % 13)[1:] - ((7 * torch.arange(300)) % 13)[:-1]).abs().min() >= 6
    assert (((5 * torch.arange(64)) % 7)[1:] - ((5 * torch.arange(64)) % 7)[:-1]).abs().min() >= 2
    assert float(max(A.abs().max(), R.abs().max())) < 60000.0


@pytest.mark.parametrize("mode", GEMM_MODES)
def test_round_to_nearest_model_is_inside_the_bound(mode):
    for M, N, K in GEMM_HOST_SHAPES:
        for epi in EPILOGUES:
            out, y, _, bound = gemm_model(M, N, K, mode, epi)
            worst, bad = elements_outside(out, y, bound)
            assert not bad, (mode, (M, N, K), epi, worst, bad)
    for case in CONV_CASES:
        for res in (False, True):
            out, y, _, bound = conv_model(case, mode, res)
            worst, bad = elements_outside(out, y, bound)
            assert not bad, (mode, case, res, worst, bad)


def violations(out, y, bound):
    return float((~((out - y).abs() <= bound)).double().mean())


# mutant -> (modes, what it is applied to): each must leave the bound on at least one of its cases
GEMM_MUTANTS = {"truncate": (("bf16", "fp16"), "plain"), "late_residual": (("bf16", "fp16"), "res"),
                "rowshift": (GEMM_MODES, "plain"), "lozero": (("bf16x3", "fp16x3"), "plain")}
CONV_MUTANTS = {"wrap": CONV_CASES[:1], "padswap": CONV_CASES[1:]}


@pytest.mark.parametrize("mutant", list(GEMM_MUTANTS))
def test_gemm_mutants_leave_the_bound(mutant):
    modes, epi = GEMM_MUTANTS[mutant]
    for mode in modes:
        share = [violations(*[gemm_model(M, N, K, mode, epi, mutant)[i] for i in (0, 1, 3)]) for M, N, K in GEMM_HOST_SHAPES]
        print(f"\n[{mutant} {mode}] share of elements outside the bound per shape: " + ", ".join(f"{s:.3f}" for s in share))
        assert max(share) > 0.0, (mutant, mode)
        if mutant in ("truncate", "rowshift", "lozero"):     # these show everywhere, not on one lucky case
            assert min(share) > 0.05, (mutant, mode, share)


@pytest.mark.parametrize("mutant", list(CONV_MUTANTS))
@pytest.mark.parametrize("mode", GEMM_MODES)
def test_conv_mutants_leave_the_bound(mutant, mode):
    for case in CONV_MUTANTS[mutant]:
        out, y, _, bound = conv_model(case, mode, False, mutant)
        share = violations(out, y, bound)
        print(f"\n[{mutant} {mode} {case}] share of elements outside the bound {share:.3f}")
        assert share > 0.0, (mutant, mode, case)


if __name__ == "__main__":
    for key, v in measured_floor().items():
        print("floor", key, f"{v:.3e}")
    for mode in GEMM_MODES:
        for M, N, K in GEMM_HOST_SHAPES:
            for epi in EPILOGUES:
                out, y, S, bound = gemm_model(M, N, K, mode, epi)
                print(f"model {mode} {(M, N, K)} {epi}: worst |err| / bound {elements_outside(out, y, bound)[0]:.3f}")
