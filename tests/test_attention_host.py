"""CPU model of the attention kernel's ARITHMETIC (csrc/attention.hip), and what tests/gpu_util.attention_row_bound is worth.

The model follows the kernel step by step in torch: fp32 scores (three products for the plane modes: the lo * lo one is
dropped), key 0 first with m = s0, l = 1, O = v0, then 64-key tiles over keys 1 .. S - 1 with one running-max update per tile,
exp2 with the 1 / 8 scale folded into the constant, P rounded to 16 bit (a hi + lo pair for the plane modes) before the PV
product, fp32 accumulation, one division at the end, and the output rounded to 16 bit (hi + lo).  What it does not model is the
order of the fp32 additions inside an MFMA and v_exp_f32's own rounding: that is the fp32 floor of the bound.

Two things are asserted, on the whole matrix of tests/test_gpu_attention.py:
  (a) the honest model stays below 1.0 of the bound: a correct kernel can meet it;
  (b) every mutant -- the model with one of the mistakes such a kernel can make -- exceeds 1.0 in the cases listed in CATCHES:
      the bound is not slack, and the inputs are such that the mistake shows.
`python -m tests.test_attention_host` prints the survey both tables were taken from."""
import functools

import pytest
import torch

from tests.gpu_util import (ATT_F32_FLOOR_FACTOR, ATT_F32_FLOOR_MEASURED, ATT_FAMILIES, ATT_MODES, ATT_PLANES, ATT_SHAPES,
                            attention_inputs, attention_planes, attention_ref64, attention_row_bound)

KT = 64                                   # keys per tile
CEXP = 0.125 * 1.4426950408889634         # softmax scale folded into exp2
MUTANTS = ("extrakey", "droplast", "key0twice", "headswap", "batchswap", "noalpha_l")


def attention_model(hi, lo, mode, mutant=None, fp32_only=False):
    """hi, lo: 16-bit planes [B, S, 3, H, 64] of the operands (lo None for bf16 / fp16).  Returns the output VALUE
    [B, S, H, 64] in fp64 (hi + lo for the plane modes).  fp32_only: P and the output stay in fp32 and every product is the
    full one -- what is left is fp32 arithmetic alone.

    mutant: extrakey   one zero key beyond S gets through the mask (score 0, v = 0)
            droplast   key S - 1 is never seen
            key0twice  l starts at 2: key 0 counted in both 32-lane halves
            headswap   V of head h - 1
            batchswap  K and V of image b ^ 1 (where it exists)
            noalpha_l  l is not rescaled when the running max grows"""
    dt, pl = ATT_PLANES[mode]
    B, S, _, H, _ = hi.shape

    def bhsd(t, which):
        return t[:, :, which].permute(0, 2, 1, 3).float().contiguous()       # [B, H, S, 64] fp32, exact

    qh, kh, vh = (bhsd(hi, i) for i in range(3))
    ql, kl, vl = (bhsd(lo, i) for i in range(3)) if pl == 2 else (None, None, None)
    if mutant == "headswap":
        vh = vh.roll(1, dims=1)
        vl = vl.roll(1, dims=1) if pl == 2 else None
    if mutant == "batchswap":
        other = torch.tensor([min(b ^ 1, B - 1) if (b ^ 1) < B else b for b in range(B)])
        kh, vh = kh[other], vh[other]
        if pl == 2:
            kl, vl = kl[other], vl[other]
    nkeys = S - 1 if (mutant == "droplast" and S > 1) else S
    if mutant == "extrakey":
        z = torch.zeros(B, H, 1, 64)
        kh, vh = torch.cat([kh, z], 2), torch.cat([vh, z], 2)
        if pl == 2:
            kl, vl = torch.cat([kl, z], 2), torch.cat([vl, z], 2)
        nkeys = S + 1
    qs = qh + ql if pl == 2 else qh                                            # unpack8x: hi + lo in fp32
    ks = kh + kl if pl == 2 else kh
    vs = vh + vl if pl == 2 else vh

    def r16(t):
        return t.to(dt).float()

    # key 0 on the VALU: the full product of the summed planes
    m = (qs * ks[:, :, :1]).sum(-1, keepdim=True)                              # [B, H, S, 1]
    l = torch.full_like(m, 2.0 if mutant == "key0twice" else 1.0)
    O = vs[:, :, :1].expand(B, H, S, 64).clone()
    for k0 in range(1, nkeys, KT):
        k1 = min(k0 + KT, nkeys)
        if pl == 2 and not fp32_only:
            s = qh @ kl[:, :, k0:k1].transpose(-1, -2) + ql @ kh[:, :, k0:k1].transpose(-1, -2) + qh @ kh[:, :, k0:k1].transpose(-1, -2)
        else:
            s = qs @ ks[:, :, k0:k1].transpose(-1, -2)
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp2((m - m_new) * CEXP)
        m = m_new
        p = torch.exp2(s * CEXP - m_new * CEXP)
        l = (l if mutant == "noalpha_l" else l * alpha) + p.sum(-1, keepdim=True)
        O = O * alpha
        if fp32_only:
            O = O + p @ vs[:, :, k0:k1]
        else:
            ph = r16(p)
            if pl == 2:
                plo = r16(p - ph)
                O = O + ph @ vl[:, :, k0:k1] + plo @ vh[:, :, k0:k1]
            O = O + ph @ vh[:, :, k0:k1]
    out = (O * (1.0 / l)).permute(0, 2, 1, 3)                                  # [B, S, H, 64] fp32
    if fp32_only:
        return out.double()
    oh = r16(out)
    return oh.double() + r16(out - oh).double() if pl == 2 else oh.double()


@functools.lru_cache(maxsize=2)
def case(mode, family, shape):
    """planes, fp64 reference and bound of one (mode, family, shape); the tests walk the matrix case by case, so the last two
    are all that is kept"""
    B, S, H = shape
    hi, lo = attention_planes(attention_inputs(B, S, H, family), mode)
    val = hi.double() + (lo.double() if lo is not None else 0.0)
    o, A, l, Vsum = attention_ref64(val)
    return hi, lo, o, A, attention_row_bound(mode, A, l, Vsum)


def worst_ratio(mode, family, shape, mutant=None):
    hi, lo, o, _, bound = case(mode, family, shape)
    return float(((attention_model(hi, lo, mode, mutant) - o).abs() / bound).max())


def fp32_floor(mode, family, shape):
    hi, lo, o, A, _ = case(mode, family, shape)
    return float(((attention_model(hi, lo, mode, fp32_only=True) - o).abs() / A).max())


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("shape", ATT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family", ATT_FAMILIES)
def test_honest_model_meets_the_row_bound(family, shape):
    for mode in ATT_MODES:
        r = worst_ratio(mode, family, shape)
        print(f"[attention model] {mode:7s} {family:9s} {shape}: worst |err| / bound {r:.3f}")
        assert r < 1.0, (mode, family, shape, r)


def test_fp32_floor_is_what_the_bound_uses():
    """the plane modes' fp32 term is ATT_F32_FLOOR_FACTOR x a floor MEASURED here, against the fp64 reference.  The constant in
    tests/gpu_util.py is that measurement (5.81e-6, fp16x3 lastkeys 2x577x12) rounded up; another CPU's matmul adds in another
    order, so this asserts that the constant is what such a measurement gives to within a factor 1.5 / 2, not the digits."""
    worst = max(fp32_floor(mode, family, shape) for mode in ("bf16x3", "fp16x3") for family in ATT_FAMILIES for shape in ATT_SHAPES)
    print(f"[attention model] fp32 floor {worst:.3e}, constant {ATT_F32_FLOOR_MEASURED:.3e} x {ATT_F32_FLOOR_FACTOR}")
    assert 0.5 * ATT_F32_FLOOR_MEASURED <= worst <= 1.5 * ATT_F32_FLOOR_MEASURED, (worst, ATT_F32_FLOOR_MEASURED)


# ---------------------------------------------------------------------------------------------------------------- (b)
BIG, FLEX, QB, SMALL, ONE = (2, 577, 12), (1, 505, 16), (3, 129, 16), (3, 65, 12), (1, 1, 12)
# The (mode, family, shape) cases this suite RELIES ON to catch each mutant: every one of them must exceed 1.0.  Taken from the
# survey (python -m tests.test_attention_host); the first of every list is the one with the least margin.  One key too many or
# too few at S >= 505 is below bf16's own rounding (0.7 - 0.9 of the bound): there the plane modes are what sees it.
CATCHES = {
    "extrakey": [("fp16", "flat", BIG), ("bf16", "flat", QB), ("fp16", "flat", FLEX), ("bf16x3", "flat", BIG), ("fp16x3", "flat", BIG),
                 ("bf16", "flat", ONE), ("fp16x3", "lastkeys", BIG)],
    "droplast": [("fp16", "flat", BIG), ("bf16", "flat", QB), ("fp16", "flat", FLEX), ("bf16x3", "flat", BIG), ("fp16x3", "flat", BIG),
                 ("bf16", "peaked", FLEX), ("bf16", "lastkeys", BIG)],
    "key0twice": [("bf16", "flat", QB), ("fp16", "flat", BIG), ("fp16", "flat", FLEX), ("bf16x3", "flat", BIG), ("fp16x3", "flat", BIG),
                  ("bf16", "flat", ONE), ("bf16", "peaked", BIG)],
    "headswap": [("bf16", "flat", BIG), ("bf16", "flat", FLEX), ("bf16", "lastkeys", ONE), ("bf16x3", "peaked", QB), ("fp16x3", "flat", BIG)],
    "batchswap": [("bf16", "flat", BIG), ("bf16", "flat", QB), ("fp16", "lastkeys", (2, 17, 16)), ("bf16x3", "peaked", SMALL),
                  ("fp16x3", "flat", BIG)],
    "noalpha_l": [("bf16", "flat", SMALL), ("bf16", "flat", BIG), ("fp16", "lastkeys", FLEX), ("bf16x3", "peaked", QB),
                  ("fp16x3", "lastkeys", (1, 2, 12))],
}


@pytest.fixture(scope="module")
def mutant_survey():
    """worst |err| / bound of every mutant on the whole matrix, case by case (one reference per case)"""
    return {(mutant, mode, family, shape): worst_ratio(mode, family, shape, mutant)
            for mode in ATT_MODES for family in ATT_FAMILIES for shape in ATT_SHAPES for mutant in MUTANTS}


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_exceeds_the_row_bound(mutant, mutant_survey):
    caught = {key[1:]: r for key, r in mutant_survey.items() if key[0] == mutant}
    n = sum(r > 1.0 for r in caught.values())
    print(f"[attention model] {mutant}: exceeds the bound in {n} of {len(caught)} cases")
    for key in CATCHES[mutant]:
        print(f"[attention model] {mutant:9s} relied on {key[0]:7s} {key[1]:9s} {key[2]}: worst |err| / bound {caught[key]:.3g}")
    for key in CATCHES[mutant]:
        assert caught[key] > 1.0, (mutant, key, caught[key])
    if mutant in ("extrakey", "droplast", "key0twice"):
        # what the flat family is for: one key too many, too few or counted twice shows in fp16 at EVERY length where it can
        # happen (up to 577), and in bf16 up to 129
        for shape in ATT_SHAPES:
            S = shape[1]
            if S < (2 if mutant == "droplast" else 1):
                continue
            assert caught[("fp16", "flat", shape)] > 1.0, (mutant, "fp16", shape, caught[("fp16", "flat", shape)])
            assert caught[("fp16x3", "flat", shape)] > 1.0 and caught[("bf16x3", "flat", shape)] > 1.0, (mutant, shape)
            if S <= 129:
                assert caught[("bf16", "flat", shape)] > 1.0, (mutant, "bf16", shape, caught[("bf16", "flat", shape)])


if __name__ == "__main__":
    import time
    t0 = time.time()
    print("fp32 floor:", max(fp32_floor(mode, family, shape) for mode in ("bf16x3", "fp16x3") for family in ATT_FAMILIES for shape in ATT_SHAPES))
    for family in ATT_FAMILIES:
        for shape in ATT_SHAPES:
            row = [f"{family:9s} {str(shape):14s}"]
            for mode in ATT_MODES:
                row.append(f"{mode} {worst_ratio(mode, family, shape):.3f}")
                for mutant in MUTANTS:
                    row.append(f"{mutant[:6]} {worst_ratio(mode, family, shape, mutant):.2g}")
                row.append("|")
            print(" ".join(row), flush=True)
    print(f"{time.time() - t0:.0f} s")
