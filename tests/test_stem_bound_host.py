"""What tests/gpu_util.stem_elem_bound, gn_elem_bound and pos_elem_bound are worth, on a CPU: the tests of
tests/test_gpu_stem_elements.py's and tests/test_gpu_glue.py's tests.

The models restate the arithmetic of the stem convolution (csrc/stem.hip), of GroupNorm (+ ReLU + max-pool) (csrc/norm.hip)
and of the position-embedding resize (csrc/misc.hip pos_resize_kernel) in plain fp32 torch:
  stem   the 13 x 133 patch as the kernel gathers it (K = (c, ky, kx) with kx padded to 8: tap 7 reads the image and meets a
         zero weight), eleven k-steps of 16 in ascending order, one fp32 addition per MFMA (three per k-step in the plane
         modes: lo hi, hi lo, hi hi), one rounding of the accumulator to the plane type (hi = rn(v), lo = rn(v - hi) for a pair);
  norm   fp32 (sum, sum of squares) per gn_chunks record, fp64 across the records, mean and rstd rounded to fp32, a = rstd
         gamma rounded, d = fma(-a, mean, beta), fma(x, a, d), the fp32 residual add, ReLU, the 3 x 3 / 2 window, one rounding;
  pos    ATen's fp32 half-pixel coordinates and the blend ly0 (lx0 a + lx1 b) + ly1 (lx0 c + lx1 d) in fp32.
What they do not model is the order of the fp32 additions inside an MFMA and inside a record: that is the fp32 floor.

Three things are asserted:
  (a) the committed floors are what the CPU measures (at least the measurement, at most twice it);
  (b) the honest models violate the bars nowhere: a correct kernel can meet them;
  (c) every mutant -- the model with one of the mistakes such a kernel can make -- leaves its bar on every shape it applies
      to: the bars are not slack, and the operands are such that the mistake shows.
`python -m tests.test_stem_bound_host` prints the survey profiles/stem_elements.md quotes."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import (GEMM_MODES, GEMM_PLANES, GN_ELEM_CASES, GN_F32_FLOOR_MEASURED, POOL_SHAPES, POS_GRIDS, STEM_IO,
                            STEM_F32_FLOOR_MEASURED, STEM_SHAPES, conv_acc64, elements_outside, gemm_operand_planes, gn_elem_bound,
                            gn_params, gn_pool_ref64, gn_ref64, plane_value, pool_operands, pos_elem_bound, pos_resize_ref64,
                            scaled_gemm_operands, scaled_pos_embed, stem_elem_bound, stem_image_planes, stem_operands,
                            stem_ref64, window_max)

EPS = 1e-5


def store(v, mode, truncate=False):
    """fp64 value of the fp32 tensor v as a kernel stores it: rounded to nearest (a pair: hi = rn(v), lo = rn(v - hi)), or --
    the mutant, one plane only -- with the low bits cut off"""
    if not truncate:
        return plane_value(gemm_operand_planes(v, mode))
    assert GEMM_PLANES[mode][1] == 1
    if mode == "bf16":
        return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32).double()
    h = v.float().half()
    over = h.float().abs() > v.float().abs()
    return (h.view(torch.int16) - over.to(torch.int16)).view(torch.float16).double()


# ------------------------------------------------------------------------------------------------------------ stem convolution
def stem_patches(x, pad_t=2, pad_l=2):
    """A [B, H/2, W/2, 176] of the image plane x [B, 3, H, W] (fp32): A[.., (c 7 + ky) 8 + kx] = x[c][2 oy + ky - pad_t]
    [2 ox + kx - pad_l], zero outside the image and in k >= 168 -- what the kernel's fragments read from its patch"""
    B, _, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    xp = F.pad(x, [pad_l, 9, pad_t, 9])
    A = torch.zeros(B, Ho, Wo, 176, dtype=x.dtype)
    A6 = A[..., :168].view(B, Ho, Wo, 3, 7, 8)
    for ky in range(7):
        for kx in range(8):
            A6[..., ky, kx] = xp[:, :, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2].permute(0, 2, 3, 1)
    return A


def stem_model32(x, wp, mode, io="fp32", mutant=None):
    """the fp32 accumulators [B, H/2, W/2, 64] of the stem kernel's arithmetic for the caller's image x [B, 3, H, W] and packed
    weight wp [64, 176] (fp64 values).  mutant: pad32, pad33 (padding (3, 2) and (3, 3) instead of TF-SAME's (2, 3): 3 rows / columns in front;
    behind the image every tap reads zero whichever it is, so at even sizes the two are one arithmetic), ky_kx (taps exchanged in the packed weight), k_order (the weight packed (ky, kx, c)), tile_shift (the patch of
    every column tile behind the first one column to the right), lo_dropped (the image's lo plane), via_bf16 (the image
    rounded to bf16 on its way into an fp16 kernel)."""
    xs = x.float().to(torch.bfloat16).float() if mutant == "via_bf16" else x
    xh, xl = stem_image_planes(xs, mode, io)
    if mutant == "lo_dropped":
        assert xl is not None
        xl = torch.zeros_like(xl)
    w4 = wp[:, :168].reshape(64, 3, 7, 8)
    if mutant == "ky_kx":
        wm = torch.zeros_like(w4)
        wm[..., :7] = w4[..., :7].transpose(2, 3)
        wp = F.pad(wm.reshape(64, 168), [0, 8])
    elif mutant == "k_order":
        wp = F.pad(w4.permute(0, 2, 3, 1).reshape(64, 168), [0, 8])
    wh, wl = gemm_operand_planes(wp, mode)
    pad = 3 if mutant in ("pad32", "pad33") else 2

    def patches(p):
        A = stem_patches(p.float(), pad, pad)
        if mutant == "tile_shift":
            A[:, :, 64:] = stem_patches(p.float(), pad, pad - 1)[:, :, 64:]
        return A.reshape(-1, 176)

    Ah, Al = patches(xh), None if xl is None else patches(xl)
    wh, wl = wh.float(), None if wl is None else wl.float()
    acc = torch.zeros(Ah.shape[0], 64)
    for ks in range(11):
        k = slice(16 * ks, 16 * ks + 16)
        if Al is not None:
            acc = acc + Al[:, k] @ wh[:, k].t()
            acc = acc + Ah[:, k] @ wl[:, k].t()
        acc = acc + Ah[:, k] @ wh[:, k].t()
    B, _, H, W = x.shape
    return acc.view(B, H // 2, W // 2, 64)


@functools.lru_cache(maxsize=None)
def stem_case(case, mode, io):
    """(x, wp, y, S, bar) of one stem case"""
    x, wp, X, Wt = stem_operands(*case)
    y, S = stem_ref64(X, Wt, mode, io)
    return x, wp, y, S, stem_elem_bound(mode, y, S)


def measured_stem_floor():
    """{(mode, io, case): largest |fp32 model - ref| / S}.  In the plane modes the reference of this measurement is the fp64
    value of the three products the kernel forms, stem_ref64's y less the lo * lo convolution: that term is not an fp32
    error, and the bar allows u^2 S for it next to the floor."""
    res = {}
    for mode in GEMM_MODES:
        for io in STEM_IO:
            for case in STEM_SHAPES:
                x, wp, y, S, _ = stem_case(case, mode, io)
                if GEMM_PLANES[mode][1] == 2:
                    _, _, X, Wt = stem_operands(*case)
                    H, W = X.shape[1], X.shape[2]
                    y = y - conv_acc64(stem_image_planes(X, mode, io)[1], gemm_operand_planes(Wt, mode)[1], 2, 2, 2, H // 2, W // 2)[0]
                res[(mode, io, case)] = float(((stem_model32(x, wp, mode, io).double() - y).abs() / S.clamp_min(1e-300)).max())
    return res


def test_stem_floor_is_what_the_bound_uses():
    worst = max(measured_stem_floor().values())
    assert worst <= STEM_F32_FLOOR_MEASURED <= 2.0 * worst, worst


@pytest.mark.parametrize("mode", GEMM_MODES)
def test_stem_honest_model_is_inside(mode):
    for io in STEM_IO:
        for case in STEM_SHAPES:
            x, wp, y, _, bar = stem_case(case, mode, io)
            worst, bad = elements_outside(store(stem_model32(x, wp, mode, io), mode), y, bar)
            assert not bad, (io, case, worst, bad)


def stem_mutants(mode, io, case):
    """the mutants that apply to one (mode, image type, shape)"""
    ms = ["pad32", "pad33", "ky_kx", "k_order"]
    if case[2] // 2 > 64:
        ms.append("tile_shift")
    if GEMM_PLANES[mode][1] == 1:
        ms.append("truncate")       # (a pair cut off twice is 2^-16 |y| off: inside what the split of a pair is allowed)
    elif io == "fp32" or (io, mode) == ("fp16", "bf16x3"):
        ms.append("lo_dropped")     # (an image of the plane type, and a bf16 image in fp16 planes, has no lo plane)
    if mode == "fp16" and io == "fp16":
        ms.append("via_bf16")
    return ms


def stem_mutant_worst(mode, io, case, mutant):
    x, wp, y, _, bar = stem_case(case, mode, io)
    acc = stem_model32(x, wp, mode, io, None if mutant == "truncate" else mutant)
    return elements_outside(store(acc, mode, mutant == "truncate"), y, bar)


@pytest.mark.parametrize("mode", GEMM_MODES)
def test_stem_mutants_leave_the_bars(mode):
    for io in STEM_IO:
        for case in STEM_SHAPES:
            for mutant in stem_mutants(mode, io, case):
                worst, bad = stem_mutant_worst(mode, io, case, mutant)
                assert bad, (io, case, mutant, worst)


# ------------------------------------------------------------------------------------------- GroupNorm (+ ReLU + max-pool)
def gn_affine32(x, gamma, beta, shift_group=0):
    """(a, d) [B, 1, C] fp32 as gn_stats_kernel and gn_affine_to_lds form them from the stored values x [B, HW, C] (fp32).
    shift_group: every channel takes the statistics of the group that many groups on (the mutant)."""
    B, HW, C = x.shape
    cpg = C // 32
    pix = min(max(16384 // C, 16), 256)
    ss = torch.zeros(B, 32, dtype=torch.float64)
    qq = torch.zeros(B, 32, dtype=torch.float64)
    for p in range(0, HW, pix):
        r = x[:, p:p + pix].reshape(B, -1, 32, cpg)
        ss += r.sum((1, 3)).double()                       # fp32 sums of one record, fp64 across records
        qq += (r * r).sum((1, 3)).double()
    n = float(HW * cpg)
    mean = ss / n
    var = (qq / n - mean * mean).clamp_min(0.0)
    eps = float(torch.tensor(EPS, dtype=torch.float32))
    mean32, rstd32 = mean.float(), (1.0 / torch.sqrt(var + eps)).float()
    if shift_group:
        mean32, rstd32 = mean32.roll(-shift_group, 1), rstd32.roll(-shift_group, 1)
    a = rstd32.repeat_interleave(cpg, 1) * gamma.float().view(1, C)
    d = (beta.double().view(1, C) - a.double() * mean32.repeat_interleave(cpg, 1).double()).float()   # fma(-a, mean, beta)
    return a.view(B, 1, C), d.view(B, 1, C)


def fma32(x, a, d):
    """fl32(x a + d) of fp32 tensors: the product is exact in fp64"""
    return (x.double() * a.double() + d.double()).float()


def gn_model32(x, gamma, beta, R=None, relu=0, mutant=None):
    """the fp32 result [B, HW, C] of gn_apply_kernel on the stored values x (and residual R), fp32 tensors"""
    a, d = gn_affine32(x, gamma, beta, 1 if mutant == "neighbour_group" else 0)
    v = fma32(torch.relu(x) if mutant == "relu_first" else x, a, d)
    if R is not None:
        v = v + R
    return torch.relu(v) if relu else v


def pool_model32(x, gamma, beta, H, W, mutant=None):
    """the fp32 result [B, H/2, W/2, C] of gn_relu_maxpool_kernel.  mutant: window_m1 (the window starts at 2 o - 1), 2x2,
    neighbour_group, relu_first."""
    B, _, C = x.shape
    v = gn_model32(x, gamma, beta, None, 0, mutant).view(B, H, W, C)
    if mutant == "window_m1":
        m = window_max(v, H, W, y_from=-1)
    elif mutant == "2x2":
        m = window_max(v, H, W, size=2)
    else:
        m = window_max(v, H, W)
    return torch.relu(m)


def stored32(x, mode):
    """the fp32 value a kernel reads back from the planes of x: hi, or fl32(hi + lo)"""
    hi, lo = gemm_operand_planes(x, mode)
    return hi.float() if lo is None else hi.float() + lo.float()


@functools.lru_cache(maxsize=None)
def pool_case(case, mode):
    """(x32, gamma, beta, y, T) of one pooling case"""
    B, H, W, C = case
    x = stored32(pool_operands(B, H, W, C, seed=C + H), mode)
    gamma, beta = gn_params(C, seed=H)
    y, T = gn_pool_ref64(x, gamma, beta, H, W, EPS)
    return x, gamma, beta, y, T


@functools.lru_cache(maxsize=None)
def gn_case(case, mode):
    """(x32, gamma, beta, R32, y, T) of one plain GroupNorm case"""
    B, HW, C, relu, res = case
    x = stored32(pool_operands(B, HW, 1, C, seed=C + HW), mode)
    gamma, beta = gn_params(C, seed=HW)
    R = stored32(scaled_gemm_operands(B * HW, C, 8, seed=C)[3].view(B, HW, C), mode) if res else None
    y, T = gn_ref64(x, gamma, beta, R, relu, EPS)
    return x, gamma, beta, R, y, T


def measured_gn_floor():
    """{(mode, case): largest |fp32 model - ref| / (2^-24 T)}"""
    res = {}
    for mode in GEMM_MODES:
        for case in POOL_SHAPES:
            x, gamma, beta, y, T = pool_case(case, mode)
            res[(mode, case)] = float(((pool_model32(x, gamma, beta, case[1], case[2]).double() - y).abs() / (2.0 ** -24 * T)).max())
        for case in GN_ELEM_CASES:
            x, gamma, beta, R, y, T = gn_case(case, mode)
            res[(mode, case)] = float(((gn_model32(x, gamma, beta, R, case[3]).double() - y).abs() / (2.0 ** -24 * T)).max())
    return res


def test_gn_floor_is_what_the_bound_uses():
    worst = max(measured_gn_floor().values())
    assert worst <= GN_F32_FLOOR_MEASURED <= 2.0 * worst, worst


@pytest.mark.parametrize("mode", GEMM_MODES)
def test_gn_honest_models_are_inside(mode):
    for case in POOL_SHAPES:
        x, gamma, beta, y, T = pool_case(case, mode)
        worst, bad = elements_outside(store(pool_model32(x, gamma, beta, case[1], case[2]), mode), y, gn_elem_bound(mode, y, T))
        assert not bad, (case, worst, bad)
    for case in GN_ELEM_CASES:
        x, gamma, beta, R, y, T = gn_case(case, mode)
        worst, bad = elements_outside(store(gn_model32(x, gamma, beta, R, case[3]), mode), y, gn_elem_bound(mode, y, T))
        assert not bad, (case, worst, bad)


POOL_MUTANTS = ("window_m1", "2x2", "neighbour_group", "relu_first", "truncate")


def pool_mutants(mode, case):
    """the mutants that apply to one (mode, shape): a 2 x 2 image has one window, which holds the whole image whichever of
    the three windows it is; a pair cut off twice is 2^-16 |y| off, inside what the split of a pair is allowed"""
    return [m for m in POOL_MUTANTS if not (m in ("window_m1", "2x2") and min(case[1], case[2]) <= 2)
            and not (m == "truncate" and GEMM_PLANES[mode][1] == 2)]


def pool_mutant_worst(mode, case, mutant):
    x, gamma, beta, y, T = pool_case(case, mode)
    v = pool_model32(x, gamma, beta, case[1], case[2], None if mutant == "truncate" else mutant)
    return elements_outside(store(v, mode, mutant == "truncate"), y, gn_elem_bound(mode, y, T))


@pytest.mark.parametrize("mode", GEMM_MODES)
def test_pool_mutants_leave_the_bars(mode):
    for case in POOL_SHAPES:
        for mutant in pool_mutants(mode, case):
            worst, bad = pool_mutant_worst(mode, case, mutant)
            assert bad, (case, mutant, worst)


# ------------------------------------------------------------------------------------------------ position-embedding resize
def pos_axis32(g_old, g, mutant=None):
    """(i0, i1, l0, l1) of one axis in the kernel's fp32 arithmetic.  mutant: align_corners (ratio (in - 1) / (out - 1), src =
    ratio dst), no_half_pixel (src = ratio dst with the half-pixel ratio)."""
    dst = torch.arange(g, dtype=torch.float32)
    if mutant == "align_corners":
        r = torch.tensor(float(g_old - 1)) / torch.tensor(float(g - 1)) if g > 1 else torch.tensor(0.0)
        s = r * dst
    else:
        r = torch.tensor(float(g_old)) / torch.tensor(float(g))
        s = r * dst if mutant == "no_half_pixel" else ((dst + 0.5) * r - 0.5).clamp_min(0.0)
    i0 = s.to(torch.int64).clamp_max(g_old - 1)
    i1 = i0 + (i0 < g_old - 1).to(torch.int64)
    l1 = s - i0.float()
    return i0, i1, 1.0 - l1, l1


def pos_model32(src, g_old, gh, gw, mutant=None):
    """the fp32 result [1 + gh gw, C] of pos_resize_kernel for src [1 + g_old^2, C] (fp32).  mutant: align_corners,
    no_half_pixel, swapped (the kernel takes gw for gh and gh for gw)."""
    if mutant == "swapped":
        gh, gw, mutant = gw, gh, None
    C = src.shape[1]
    G = src[1:].view(g_old, g_old, C)
    y0, y1, ly0, ly1 = pos_axis32(g_old, gh, mutant)
    x0, x1, lx0, lx1 = pos_axis32(g_old, gw, mutant)
    ly0, ly1 = ly0.view(-1, 1, 1), ly1.view(-1, 1, 1)
    lx0, lx1 = lx0.view(1, -1, 1), lx1.view(1, -1, 1)
    v = ly0 * (lx0 * G[y0][:, x0] + lx1 * G[y0][:, x1]) + ly1 * (lx0 * G[y1][:, x0] + lx1 * G[y1][:, x1])
    return torch.cat([src[:1], v.reshape(-1, C)])


@functools.lru_cache(maxsize=None)
def pos_case(grid, C):
    src = scaled_pos_embed(C, seed=C)
    y, Sb, L = pos_resize_ref64(src, 24, *grid)
    return src.float(), y, pos_elem_bound(Sb, L)


@pytest.mark.parametrize("C", [768, 1024])
def test_pos_honest_model_is_inside_and_mutants_leave(C):
    src = scaled_pos_embed(C, seed=C).float()
    assert torch.equal(pos_model32(src, 24, 24, 24), src)            # the identity: weights 1 and 0 are exact
    for grid in POS_GRIDS:
        src, y, bar = pos_case(grid, C)
        worst, bad = elements_outside(pos_model32(src, 24, *grid), y, bar)
        assert not bad, (grid, worst, bad)
        for mutant in ("align_corners", "no_half_pixel") + (("swapped",) if grid[0] != grid[1] else ()):
            worst, bad = elements_outside(pos_model32(src, 24, *grid, mutant), y, bar)
            assert bad, (grid, mutant, worst)


def survey():
    sf = measured_stem_floor()
    print("stem fp32 floor, largest |model32 - ref| / S per mode (over image types and shapes):")
    for mode in GEMM_MODES:
        print(f"  {mode:7s} {max(v for k, v in sf.items() if k[0] == mode):.3e}")
    print("stem honest model, worst |err| / bar per mode; mutants, smallest worst |err| / bar over the shapes they apply to:")
    for mode in GEMM_MODES:
        h = max(elements_outside(store(stem_model32(*stem_case(c, mode, io)[:2], mode, io), mode), *stem_case(c, mode, io)[2:5:2])[0]
                for io in STEM_IO for c in STEM_SHAPES)
        row = {}
        for io in STEM_IO:
            for c in STEM_SHAPES:
                for m in stem_mutants(mode, io, c):
                    row[m] = min(row.get(m, float("inf")), stem_mutant_worst(mode, io, c, m)[0])
        print(f"  {mode:7s} honest {h:.3f}  " + "  ".join(f"{m} {v:.3g}" for m, v in row.items()))
    gf = measured_gn_floor()
    print("GroupNorm fp32 floor in units of 2^-24 T per mode: pool shapes / plain cases")
    for mode in GEMM_MODES:
        print(f"  {mode:7s} {max(v for k, v in gf.items() if k[0] == mode and len(k[1]) == 4):.2f} / "
              f"{max(v for k, v in gf.items() if k[0] == mode and len(k[1]) == 5):.2f}")
    print("pool honest model, worst |err| / bar per mode; mutants, smallest worst |err| / bar over the shapes:")
    for mode in GEMM_MODES:
        h = 0.0
        for c in POOL_SHAPES:
            x, gamma, beta, y, T = pool_case(c, mode)
            h = max(h, elements_outside(store(pool_model32(x, gamma, beta, c[1], c[2]), mode), y, gn_elem_bound(mode, y, T))[0])
        row = {}
        for c in POOL_SHAPES:
            for m in pool_mutants(mode, c):
                row[m] = min(row.get(m, float("inf")), pool_mutant_worst(mode, c, m)[0])
        print(f"  {mode:7s} honest {h:.3f}  " + "  ".join(f"{m} {v:.3g}" for m, v in row.items()))
    print("pos_resize honest model, worst |err| / bar; mutants, smallest worst |err| / bar over the grids:")
    for C in (768, 1024):
        h = max(elements_outside(pos_model32(pos_case(g, C)[0], 24, *g), *pos_case(g, C)[1:])[0] for g in POS_GRIDS)
        row = {m: min(elements_outside(pos_model32(pos_case(g, C)[0], 24, *g, m), *pos_case(g, C)[1:])[0]
                      for g in POS_GRIDS if m != "swapped" or g[0] != g[1]) for m in ("align_corners", "no_half_pixel", "swapped")}
        print(f"  C={C} honest {h:.3f}  " + "  ".join(f"{m} {v:.3g}" for m, v in row.items()))


if __name__ == "__main__":
    survey()
