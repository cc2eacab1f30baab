"""What tests/gpu_util.up_elem_bound and head_elem_bound are worth, on a CPU: the tests of tests/test_gpu_head_elements.py's tests.

The models restate the arithmetic of the x2 up-sampling (csrc/misc.hip) and of the head tail (csrc/head.hip) in plain fp32
torch: ATen's fp32 indices and weights (either rounding of l1, gpu_util.up_axis32), the blend ly0 (lx0 a + lx1 b) + ly1 (lx0 c +
lx1 d), ONE rounding of the fp32 blend to the plane type (hi = rn(v), lo = rn(v - hi) for a pair), the 3x3 convolution on the
stored window (three products for a pair, lo * lo dropped) per 32-column tile with its one-pixel halo, + b2, ReLU, the 32-term
projection + b4, ReLU.  What they do not model is the order of the fp32 additions inside an MFMA and the fused multiply-adds:
that is the fp32 floor of the bounds.

Three things are asserted:
  (a) the committed floor of the blend is what the CPU measures with F.interpolate in fp32 (at least the measurement, at most
      twice it), and the fp32 head chain stays inside its bound with the GEMM floor;
  (b) the honest models violate the bounds nowhere: a correct kernel can meet them;
  (c) every mutant -- the model with one of the mistakes such a kernel can make -- leaves the bound: the bounds are not slack,
      and the operands are such that the mistake shows.
`python -m tests.test_head_bound_host` prints the survey profiles/head_elements.md quotes."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import (GEMM_F32_FLOOR_FACTOR, GEMM_F32_FLOOR_MEASURED, GEMM_MODES, GEMM_PLANES, HEAD_HOST_SHAPES,
                            UP_F32_FLOOR_MEASURED, UP_HOST_CASES, UP_VARIANTS, elements_outside, gemm_operand_planes,
                            head_elem_bound, head_tail_ref64, scaled_head_operands, up_axis32, up_elem_bound, upsample_ref64,
                            upsample_variants_inside)

HEAD_MODES = ("bf16", "fp16", "fp16x3")
NAN = float("nan")


def planes(x, mode):
    """(hi, lo) fp32 tensors holding the plane values of x; lo is None in the one-plane modes"""
    hi, lo = gemm_operand_planes(x, mode)
    return hi.float(), None if lo is None else lo.float()


def value(p):
    return p[0].double() if p[1] is None else p[0].double() + p[1].double()


def store(v, mode):
    """(hi, lo) of the fp32 tensor v as a kernel stores it"""
    return planes(v, mode)


def up_model32(X32, variant, mutant=None):
    """the blend of fp32 values X32 [B, H, W, C] in fp32.  mutant: half_pixel (align_corners=False ratios), y1_unclamped (row
    y0 + 1 of the flat row array, whatever lies there -- NaN behind the last image, as the GPU test places it), lx_swapped."""
    B, H, W, C = X32.shape

    def axis(n, fma):
        i0, i1, l0, l1 = up_axis32(n, fma)
        if mutant == "half_pixel":
            src = ((torch.arange(2 * n, dtype=torch.float32) + 0.5) * 0.5 - 0.5).clamp_min(0.0)
            i0 = src.to(torch.int64)
            i1 = i0 + (i0 < n - 1).to(torch.int64)
            l1 = src - i0.float()
            l0 = 1.0 - l1
        return i0, i1, l0, l1

    y0, y1, ly0, ly1 = axis(H, bool(variant & 2))
    x0, x1, lx0, lx1 = axis(W, bool(variant & 1))
    if mutant == "lx_swapped":
        lx0, lx1 = lx1, lx0
    if mutant == "y1_unclamped":
        rows = torch.cat([X32.reshape(B * H, W, C), torch.full((1, W, C), NAN)])
        base = (torch.arange(B) * H).view(B, 1)
        r0, r1 = rows[base + y0.view(1, -1)], rows[base + y0.view(1, -1) + 1]
    else:
        r0, r1 = X32[:, y0], X32[:, y1]
    ly0, ly1 = ly0.view(1, -1, 1, 1), ly1.view(1, -1, 1, 1)
    lx0, lx1 = lx0.view(1, 1, -1, 1), lx1.view(1, 1, -1, 1)
    return ly0 * (lx0 * r0[:, :, x0] + lx1 * r0[:, :, x1]) + ly1 * (lx0 * r1[:, :, x0] + lx1 * r1[:, :, x1])


@functools.lru_cache(maxsize=None)
def up_case(case, mode):
    """(planes of the input, its fp64 value) of one up-sampling case"""
    B, H, W, C = case
    p = planes(scaled_head_operands(B, H, W, 1, 0, C)[0], mode)
    return p, value(p)


def up_inside(out, Xv, mode):
    """(worst |err| / bound per variant, set of variants of the reference that hold every element) of the stored planes `out`"""
    return upsample_variants_inside(value(out), Xv, mode)


@functools.lru_cache(maxsize=None)
def up_refs(case, mode):
    """(y, bound) of the four variants of one of the small cases"""
    Xv = up_case(case, mode)[1]
    return [(y, up_elem_bound(mode, y, Sb)) for y, Sb in (upsample_ref64(Xv, v) for v in range(4))]


def measured_up_floor():
    """{(mode, case): (largest |F.interpolate(fp32) - ref| / (2^-24 Sb) against the variant that fits best, that variant)}"""
    res = {}
    for mode in GEMM_MODES:
        for case in UP_HOST_CASES:
            p, Xv = up_case(case, mode)
            x32 = Xv.float()            # hi + lo is an fp32 number
            assert torch.equal(x32.double(), Xv)
            ref32 = F.interpolate(x32.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
            best = None
            for v in range(4):
                y, Sb = upsample_ref64(Xv, v)
                r = float(((ref32.double() - y).abs() / (2.0 ** -24 * Sb).clamp_min(1e-300)).max())
                best = (r, v) if best is None or r < best[0] else best
            res[(mode, case)] = best
    return res


def test_up_floor_is_what_the_bound_uses():
    worst = max(r for r, _ in measured_up_floor().values())
    assert worst <= UP_F32_FLOOR_MEASURED <= 2.0 * worst, worst


@pytest.mark.parametrize("mode", GEMM_MODES)
def test_fp32_interpolate_and_model_are_inside_the_up_bound(mode):
    """F.interpolate in fp32 and the model, rounded to the planes, against the bound: each inside for one variant throughout"""
    for case in UP_HOST_CASES[:3]:
        p, Xv = up_case(case, mode)
        ref32 = F.interpolate(Xv.float().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        worst, inside = up_inside(store(ref32, mode), Xv, mode)
        assert inside, (mode, case, worst)
        for v in range(4):
            worst, inside = up_inside(store(up_model32(Xv.float(), v), mode), Xv, mode)
            assert v in inside, (mode, case, UP_VARIANTS[v], worst)


UP_MUTANTS = ("half_pixel", "y1_unclamped", "lx_swapped", "lo_dropped")


@pytest.mark.parametrize("mutant", UP_MUTANTS)
def test_up_mutants_leave_the_bound(mutant):
    """no variant of the reference accepts a mutant, whichever l1 the mutant itself uses"""
    for mode in (("bf16x3", "fp16x3") if mutant == "lo_dropped" else GEMM_MODES):
        for case in UP_HOST_CASES[:2]:
            p, Xv = up_case(case, mode)
            for v in range(4):
                x32 = p[0] if mutant == "lo_dropped" else Xv.float()
                out = value(store(up_model32(x32, v, None if mutant == "lo_dropped" else mutant), mode))
                for r, (y, bound) in enumerate(up_refs(case, mode)):
                    assert elements_outside(out, y, bound)[1], (mutant, mode, case, UP_VARIANTS[v], "accepted by", UP_VARIANTS[r])


# ---------------------------------------------------------------------------------------------------------------- head tail
def conv32_tiles(U, W, mutant=None):
    """3x3 pad-1 convolution in fp32 of U [B, Ho, Wo, 128] with W [32, 3, 3, 128], one 32-column tile at a time on its 34-column
    window, as head.hip builds it -> [B, Ho, Wo, 32].  mutant: shift (the window starts one column too far left), replicate (edge
    replication instead of zero padding), wrong_halo (the left halo column of the second tile comes from the next image)."""
    B, Ho, Wo, _ = U.shape
    x = U.permute(0, 3, 1, 2)
    if mutant == "replicate":
        xp = F.pad(x, [1, 1, 1, 1], mode="replicate")
    else:
        xp = F.pad(x, [1, 1, 1, 1])
    if mutant == "shift":
        xp = F.pad(xp, [1, 0, 0, 0])[..., :-1]
    w = W.permute(0, 3, 1, 2)
    out = []
    for tx in range(Wo // 32):
        win = xp[..., tx * 32:tx * 32 + 34].clone()
        if mutant == "wrong_halo" and tx == 1:
            win[..., 0] = win[..., 0].roll(-1, 0)
        out.append(F.conv2d(win, w))
    return torch.cat(out, -1).permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=None)
def head_case(shape, mode):
    """the operands of one head case: planes of H0 and W2, the fp32 vectors, the stored up-sampled window (planes) of the
    honest model and the fp64 reference pieces from it"""
    B, Hs, Ws, C, relu = shape
    H0, W2, b2, w4, b4 = scaled_head_operands(B, Hs, Ws, C)
    hp, wp = planes(H0, mode), planes(W2, mode)
    b2, w4, b4 = b2.float(), w4.float(), b4.float()
    U = store(up_model32(value(hp).float(), 3), mode)
    return hp, wp, b2, w4, b4, U, head_tail_ref64(value(U), value(wp), b2, w4, b4, relu)


def head_model(shape, mode, mutant=None):
    """(fp32 result NCHW, y, bound) of one case of the model; mutants as listed in HEAD_MUTANTS"""
    B, Hs, Ws, C, relu = shape
    hp, wp, b2, w4, b4, U, (y, Sw, Hw, _) = head_case(shape, mode)
    if mutant == "lo_dropped":
        U = store(up_model32(hp[0], 3), mode)
    # ulp: the LARGEST window element one 16-bit step up.  The bound sees it only in the few outputs that element dominates (shares
    # down to 0.0002); a flipped rounding of a small element next to large ones is, by construction, below F (Sw + Hw) everywhere
    # and visible only to the bitwise window probe (tests/test_gpu_head_elements.py test_head_window_probe)
    if mutant == "ulp":
        uh = U[0].clone()
        i = int(uh.abs().argmax())
        dt = GEMM_PLANES[mode][0]
        uh.view(-1)[i] = (uh.view(-1)[i:i + 1].to(dt).view(torch.int16) + 1).view(dt).float()
        U = (uh, U[1])
    cm = mutant if mutant in ("shift", "replicate", "wrong_halo") else None
    if U[1] is None:
        acc = conv32_tiles(U[0], wp[0], cm)
    else:
        acc = conv32_tiles(U[0], wp[1], cm) + conv32_tiles(U[1], wp[0], cm) + conv32_tiles(U[0], wp[0], cm)
    h = F.relu(acc) + b2 if mutant == "late_bias" else F.relu(acc + b2)
    w = w4[[2, 1, 0]] if mutant == "w4_swapped" else w4
    out = h @ w.t() + b4
    if relu:
        out = F.relu(out)
    return out.permute(0, 3, 1, 2), y, head_elem_bound(mode, y, Sw, Hw), Sw + Hw


def measured_head_floor():
    """{(mode, shape): largest |fp32 chain - fp64| / (GEMM_F32_FLOOR_MEASURED (Sw + Hw)) of the honest model}"""
    res = {}
    for mode in HEAD_MODES:
        for shape in HEAD_HOST_SHAPES:
            out, y, _, S = head_model(shape, mode)
            res[(mode, shape)] = float(((out.double() - y).abs() / (GEMM_F32_FLOOR_MEASURED * S)).max())
    return res


def test_head_floor_is_inside_the_margin():
    """the fp32 chain on a CPU needs no more than the GEMM floor's margin (the bound's u^2 term of fp16x3 left aside)"""
    worst = max(measured_head_floor().values())
    assert worst <= GEMM_F32_FLOOR_FACTOR, worst


@pytest.mark.parametrize("mode", HEAD_MODES)
def test_head_model_is_inside_the_bound(mode):
    for shape in HEAD_HOST_SHAPES:
        out, y, bound, _ = head_model(shape, mode)
        worst, bad = elements_outside(out, y, bound)
        assert not bad, (mode, shape, worst, bad)


def violations(out, y, bound):
    return float((~((out.double() - y).abs() <= bound)).double().mean())


# mutant -> (modes, shapes it is applied to)
HEAD_MUTANTS = {"shift": (HEAD_MODES, HEAD_HOST_SHAPES), "replicate": (HEAD_MODES, HEAD_HOST_SHAPES),
                "ulp": (HEAD_MODES, HEAD_HOST_SHAPES), "lo_dropped": (("fp16x3",), HEAD_HOST_SHAPES),
                "late_bias": (HEAD_MODES, HEAD_HOST_SHAPES), "w4_swapped": (HEAD_MODES, (HEAD_HOST_SHAPES[1], HEAD_HOST_SHAPES[3])),
                "wrong_halo": (HEAD_MODES, (HEAD_HOST_SHAPES[1], HEAD_HOST_SHAPES[3]))}


@pytest.mark.parametrize("mutant", list(HEAD_MUTANTS))
def test_head_mutants_leave_the_bound(mutant):
    modes, shapes = HEAD_MUTANTS[mutant]
    for mode in modes:
        share = []
        for shape in shapes:
            out, y, bound, _ = head_model(shape, mode, mutant)
            share.append(violations(out, y, bound))
        print(f"\n[{mutant} {mode}] share of elements outside the bound per shape: " + ", ".join(f"{s:.4f}" for s in share))
        assert min(share) > 0.0, (mutant, mode, share)


if __name__ == "__main__":
    for key, (r, v) in measured_up_floor().items():
        print("up floor", key, f"{r:.2f} x 2^-24 Sb against {UP_VARIANTS[v]}")
    for key, r in measured_head_floor().items():
        print("head floor", key, f"{r:.3f} x {GEMM_F32_FLOOR_MEASURED} (Sw + Hw)")
    for mode in GEMM_MODES:
        for case in UP_HOST_CASES:
            p, Xv = up_case(case, mode)
            ref32 = F.interpolate(Xv.float().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
            worst, inside = up_inside(store(ref32, mode), Xv, mode)
            print(f"up {mode} {case}: F.interpolate rounded, worst |err| / bound per variant "
                  + ", ".join(f"{worst[v]:.3f}" for v in range(4)) + f"; inside {sorted(inside)}")
    for mode in HEAD_MODES:
        for shape in HEAD_HOST_SHAPES:
            out, y, bound, S = head_model(shape, mode)
            print(f"head {mode} {shape}: worst |err| / bound {elements_outside(out, y, bound)[0]:.3f}; "
                  f"median bound / |y| over y != 0 {float((bound / y.abs())[y != 0].median()):.2e}")
