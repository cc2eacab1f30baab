"""What the bars of tests/gpu_util's conv + GroupNorm record section (conv_gn_stats64, gn_tables_ref64, gn_records_out_ref64)
are worth, on a CPU: the tests of tests/test_gpu_gn_records_elements.py's tests.

The model restates the arithmetic of the chain in plain fp32 torch:
  records   csrc/gemm_impl.h gn_records on a 32 x 32 accumulator block (lane = column, lane half lh and register r hold row
            8 (r / 4) + 4 lh + r % 4): per lane 16 registers in sequence, the squares with fmaf; then lane ^ 32 (the two halves);
            then lane ^ 1 .. cpg / 2 (a pairwise tree over the group's columns);
  affines   csrc/norm.hip gn_affine_to_lds: fp64 across the records in 8 slices (slice s takes records s, s + 8, ...), the slices
            combined in order, mean and rstd rounded to fp32, a = rstd gamma rounded, d = fma(-a, mean, beta);
  apply     gn_apply_kernel / the C1_GN epilogue: fma(x, a, d), the shortcut as it is or as fma(R, ra, rd), one rounded add,
            ReLU, one rounding to the plane type.
Its accumulators are the fp64 ones rounded to fp32; what it does not model is the order of the additions inside the MFMAs,
which the accumulator bar E of conv_gn_stats64 stands for.

Three things are asserted:
  (a) the committed constants are what the CPU measures (at least the measurement, at most twice it);
  (b) the honest model violates no bar, in all four modes: a correct kernel can meet them;
  (c) every mutant -- the model with one of the mistakes such a chain can make -- leaves its bar on at least one case: the bars
      are not slack, and the operands are such that the mistake shows.
`python -m tests.test_gn_records_bound_host` prints the survey profiles/gn_records_elements.md quotes."""
import functools

import pytest
import torch

from tests.gpu_util import (GEMM_MODES, GEMM_PLANES, GNREC_APPLY_HOST, GNREC_CA_MEASURED, GNREC_CASES, GNREC_CM_MEASURED,
                            GNREC_CQ_MEASURED, GNREC_CS_MEASURED, GNREC_U, assert_r_coverage, conv_acc64, conv_gn_geometry,
                            conv_gn_operands, conv_gn_stats64, elements_outside, gemm_operand_planes, gn_map_operands,
                            gn_records_out_ref64, gn_tables_ref64, plane_value, records_of, stats_of_records)
from tests.test_stem_bound_host import fma32, store, stored32

EPS = 1e-5
RECORD_MUTANTS = ("blk_plus_1", "last_dropped", "neighbour_group", "half_rows")
TABLE_MUTANTS = ("prev_image", "var_fp32", "no_beta")
OUTPUT_MUTANTS = ("main_table", "relu_first", "truncate")


# ------------------------------------------------------------------------------------------------------------ the fp32 model
def records_model32(v, mutant=None):
    """records [B, HW / 32, 32, 2] fp32 of the accumulators v [B, HW, C] (fp32) in gn_records' order; a record the mutant does
    not write stays NaN.  mutant: blk_plus_1 (written one block late), last_dropped (the last block of every image),
    neighbour_group (group g ^ 1's sums), half_rows (lane ^ 32 skipped)."""
    B, HW, C = v.shape
    cpg, nblk = C // 32, HW // 32
    t = v.float().reshape(B, nblk, 4, 2, 4, C)               # row = 8 (r / 4) + 4 lh + r % 4
    sm = torch.zeros(B, nblk, 2, C)
    sq = torch.zeros(B, nblk, 2, C)
    for r in range(16):
        x = t[:, :, r // 4, :, r % 4, :]
        sm = sm + x
        sq = fma32(x, x, sq)
    if mutant == "half_rows":
        sm, sq = sm[:, :, 0], sq[:, :, 0]
    else:
        sm, sq = sm[:, :, 0] + sm[:, :, 1], sq[:, :, 0] + sq[:, :, 1]
    o = 1
    while o < cpg:                                           # lane ^ o: adjacent partial sums pair up
        sm = sm.reshape(B, nblk, -1, 2)
        sq = sq.reshape(B, nblk, -1, 2)
        sm, sq = sm[..., 0] + sm[..., 1], sq[..., 0] + sq[..., 1]
        o *= 2
    rec = torch.stack([sm, sq], -1)
    if mutant == "neighbour_group":
        rec = rec[:, :, torch.arange(32) ^ 1]
    elif mutant == "last_dropped":
        rec[:, -1] = float("nan")
    elif mutant == "blk_plus_1":
        rec = torch.cat([torch.full_like(rec[:, :1], float("nan")), rec[:, :-1]], 1)
    return rec.contiguous()


def affine_model32(rec, gamma, beta, HW, mutant=None):
    """(a, d, mean32, rstd32): a, d [B, C] fp32 as gn_affine_to_lds forms them from the records [B, nrec, 32, 2].  mutant:
    prev_image (every image takes the rows of the image before it), var_fp32 (the sums across the records, the moments and
    E[x^2] - mean^2 in fp32 instead of fp64), no_beta (d = -a mean on the channels whose scale is 1/8)."""
    B, nrec = rec.shape[:2]
    C = gamma.numel()
    cpg = C // 32
    acc_t = torch.float32 if mutant == "var_fp32" else torch.float64
    tot = torch.zeros(B, 32, 2, dtype=acc_t)
    for s in range(8):
        part = torch.zeros(B, 32, 2, dtype=acc_t)
        for c in range(s, nrec, 8):
            part = part + rec[:, c].to(acc_t)
        tot = tot + part
    n = torch.tensor(float(HW * cpg), dtype=acc_t)
    mean = tot[..., 0] / n
    var = (tot[..., 1] / n - mean * mean).clamp_min(0.0)
    eps = float(torch.tensor(EPS, dtype=torch.float32))
    mean32, rstd32 = mean.float(), (1.0 / torch.sqrt(var.double() + eps)).float()
    a = rstd32.repeat_interleave(cpg, 1) * gamma.float().view(1, C)
    be = beta.float().view(1, C).expand(B, C)
    if mutant == "no_beta":
        small = ((5 * torch.arange(C)) % 7 - 3) == -3
        be = torch.where(small.view(1, C), torch.zeros_like(be), be)
    d = fma32(-a, mean32.repeat_interleave(cpg, 1), be)
    if mutant == "prev_image":
        a, d = a.roll(1, 0), d.roll(1, 0)
    return a, d, mean32, rstd32


def apply_model32(x, a, d, R=None, ra=None, rd=None, relu=0, mutant=None):
    """the fp32 result [B, HW, C] of the apply pass on the stored values x, R (fp32).  mutant: main_table (the shortcut
    normalised with (a, d)), relu_first (ReLU before the shortcut is added)."""
    B, HW, C = x.shape
    f = fma32(x, a.view(B, 1, C).expand_as(x), d.view(B, 1, C).expand_as(x))
    if mutant == "relu_first" and relu:
        f = torch.relu(f)
    if R is not None:
        r = R
        if ra is not None:
            ta, td = (a, d) if mutant == "main_table" else (ra, rd)
            r = fma32(R, ta.view(B, 1, C).expand_as(R), td.view(B, 1, C).expand_as(R))
        f = f + r
    return torch.relu(f) if relu else f


# ------------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def branch(case, mode, seed):
    """one convolution of a case: (v32 [B, HW, C] the accumulators rounded to fp32, statistics dict, gamma, beta (fp32), R64)"""
    B, H, W, Cin, Cout, k, stride = case
    pad, Ho, Wo = conv_gn_geometry(case)
    X, Wt, gamma, beta, R = conv_gn_operands(B, H, W, Cin, Cout, k, stride, seed)
    acc, S = conv_acc64(plane_value(gemm_operand_planes(X, mode)), plane_value(gemm_operand_planes(Wt, mode)), stride, pad, pad, Ho, Wo)
    st = conv_gn_stats64(mode, acc, S, EPS)
    return acc.float().reshape(B, Ho * Wo, Cout), st, gamma.float(), beta.float(), R.reshape(B, Ho * Wo, Cout)


def case_seed(case):
    return case[3] + case[4] + 7 * case[5] + case[0]


def honest_tables(case, mode, second=False, mutant=None):
    v, st, gamma, beta, _ = branch(case, mode, case_seed(case) + (1 if second else 0))
    rec = records_model32(v)
    return affine_model32(rec, gamma, beta, v.shape[1], mutant)


def output_of(case, mode, res, relu, mutant=None):
    """(stored model output, y, bound) of one apply: res 0 none, 1 plain R, 2 the second convolution behind its GroupNorm"""
    v, st, gamma, beta, R = branch(case, mode, case_seed(case))
    a, d, _, _ = honest_tables(case, mode)
    x = stored32(v, mode)                                    # the raw map as stored and read back
    tab = gn_tables_ref64(st, gamma, beta)
    Rs, ra, rd, rtab = None, None, None, None
    if res == 1:
        Rs = stored32(R, mode)
    elif res == 2:
        v2, st2, g2, b2, _ = branch(case, mode, case_seed(case) + 1)
        Rs = stored32(v2, mode)
        ra, rd, _, _ = honest_tables(case, mode, second=True)
        rtab = gn_tables_ref64(st2, g2, b2)
    y, bound = gn_records_out_ref64(mode, x, tab, Rs, rtab, relu)
    out = apply_model32(x, a, d, Rs, ra, rd, relu, None if mutant == "truncate" else mutant)
    return store(out, mode, mutant == "truncate"), y, bound


def test_cases_cover_the_ratios():
    for mode in GEMM_MODES:
        for case in GNREC_CASES:
            for second in (0, 1):
                assert_r_coverage(branch(case, mode, case_seed(case) + second)[1])


# ------------------------------------------------------------------------------------------------------------ (a) constants
def measured_constants():
    """{name: {(mode, case): largest ratio}} of the honest model to the reference, the accumulator bar E left out: the model's
    accumulators are the reference's, rounded to fp32"""
    res = {"c_s": {}, "c_q": {}, "c_a": {}, "c_m": {}}
    u = GNREC_U

    def take(key, rec, ref_rec, Sabs, mean32, rstd32, st):
        res["c_s"][key] = float(((rec[..., 0].double() - ref_rec[..., 0]).abs() / (u * Sabs)).max())
        res["c_q"][key] = float(((rec[..., 1].double() - ref_rec[..., 1]).abs() / (u * ref_rec[..., 1])).max())
        rstd = 1.0 / st["sigma"]
        res["c_a"][key] = float(((rstd32.double() - rstd).abs() / rstd / (u * (1.0 + st["r"] ** 2))).max())
        res["c_m"][key] = float(((mean32.double() - st["mean"]).abs() / (u * (1.0 + st["r"]) * st["sigma"])).max())

    for mode in GEMM_MODES:
        for case in GNREC_CASES:
            for second in (0, 1):
                v, st, gamma, beta, _ = branch(case, mode, case_seed(case) + second)
                B, HW, C = v.shape
                rec = records_model32(v)
                _, _, mean32, rstd32 = affine_model32(rec, gamma, beta, HW)
                Sabs = st["v"].abs().reshape(B, HW // 32, 32, 32, C // 32).sum((2, 4))
                take((mode, case, second), rec, st["rec"], Sabs, mean32, rstd32, st)
        for shape in GNREC_APPLY_HOST:
            B, HW, C = shape
            x = gn_map_operands(B, HW, C, seed=HW + C)[0]
            v = plane_value(gemm_operand_planes(x, mode)).float()
            st = map_stats(v.double())
            rec = records_model32(v)
            _, _, mean32, rstd32 = affine_model32(rec, torch.ones(C), torch.zeros(C), HW)
            Sabs = v.double().abs().reshape(B, HW // 32, 32, 32, C // 32).sum((2, 4))
            take((mode, shape, 0), rec, st["rec"], Sabs, mean32, rstd32, st)
    return res


def map_stats(v):
    """conv_gn_stats64 of a map taken as exact accumulators (S = |v|, E irrelevant to the measurement)"""
    return conv_gn_stats64("bf16", v.unsqueeze(1), v.abs().unsqueeze(1), EPS)


def test_record_constants_are_what_the_bounds_use():
    m = measured_constants()
    for name, const in (("c_s", GNREC_CS_MEASURED), ("c_q", GNREC_CQ_MEASURED), ("c_a", GNREC_CA_MEASURED), ("c_m", GNREC_CM_MEASURED)):
        worst = max(m[name].values())
        assert worst <= const <= 2.0 * worst, (name, worst, const)


# ------------------------------------------------------------------------------------------------------- (b) the honest model
@pytest.mark.parametrize("mode", GEMM_MODES)
def test_honest_model_is_inside(mode):
    for case in GNREC_CASES:
        for second in (0, 1):
            v, st, gamma, beta, _ = branch(case, mode, case_seed(case) + second)
            rec = records_model32(v)
            worst, bad = elements_outside(rec, st["rec"], st["rec_bar"])
            assert not bad, (case, second, "records", worst, bad)
            a, d, _, _ = affine_model32(rec, gamma, beta, v.shape[1])
            tab = gn_tables_ref64(st, gamma, beta)
            for got, ref, bar, what in ((a, tab["a"], tab["a_bar"], "a"), (d, tab["d"], tab["d_bar"], "d")):
                worst, bad = elements_outside(got, ref, bar)
                assert not bad, (case, second, what, worst, bad)
        for res in (0, 1, 2):
            for relu in (0, 1):
                worst, bad = elements_outside(*output_of(case, mode, res, relu))
                assert not bad, (case, res, relu, worst, bad)


@pytest.mark.parametrize("mode", GEMM_MODES)
def test_honest_apply_from_exact_records_is_inside(mode):
    """the apply pass alone, as tests/test_gpu_gn_records_elements.py runs it: fp64 records rounded to fp32"""
    for shape in GNREC_APPLY_HOST:
        B, HW, C = shape
        x64, gamma, beta, R = gn_map_operands(B, HW, C, seed=HW + C)
        x, Rs = stored32(x64, mode), stored32(R, mode)
        rec = records_of(x)
        tab = gn_tables_ref64(stats_of_records(rec, HW, C // 32, EPS), gamma.float(), beta.float())
        a, d, _, _ = affine_model32(rec, gamma.float(), beta.float(), HW)
        for got, ref, bar, what in ((a, tab["a"], tab["a_bar"], "a"), (d, tab["d"], tab["d_bar"], "d")):
            worst, bad = elements_outside(got, ref, bar)
            assert not bad, (shape, what, worst, bad)
        y, bound = gn_records_out_ref64(mode, x, tab, Rs, None, 1)
        worst, bad = elements_outside(store(apply_model32(x, a, d, Rs, relu=1), mode), y, bound)
        assert not bad, (shape, worst, bad)


# --------------------------------------------------------------------------------------------------------------- (c) mutants
def mutant_cases(mutant, mode):
    """the cases a mutant applies to.  var_fp32 is judged where the statistics' bar is tight -- on records that are exact
    (GNREC_APPLY_HOST; on the GPU: test_tables_from_exact_records), a bar of 2 u on a --: behind a convolution the bar must
    allow for accumulators that are all off by F S in one direction, which moves the variance by more than its formation in
    fp32 does (the survey prints it: 0 of 19 cases)."""
    if mutant == "var_fp32":
        return list(GNREC_APPLY_HOST)
    cases = list(GNREC_CASES)
    if mutant in ("blk_plus_1", "prev_image"):
        cases = [c for c in cases if c[0] > 1]                # (one record: the late one falls behind the tensor, into the guard)
    if mutant == "neighbour_group":
        cases = [c for c in cases if c[4] == 64]
    return cases if not (mutant == "truncate" and GEMM_PLANES[mode][1] == 2) else []


def mutant_worst(mutant, mode, case):
    """worst |err| / bar of a mutant on the bar that is to reject it"""
    if len(case) == 3:                                        # (B, HW, C): tables from exact records
        B, HW, C = case
        x64, gamma, beta, _ = gn_map_operands(B, HW, C, seed=HW + C)
        rec = records_of(stored32(x64, mode))
        tab = gn_tables_ref64(stats_of_records(rec, HW, C // 32, EPS), gamma.float(), beta.float())
        a, d, _, _ = affine_model32(rec, gamma.float(), beta.float(), HW, mutant)
        return max(elements_outside(a, tab["a"], tab["a_bar"])[0], elements_outside(d, tab["d"], tab["d_bar"])[0])
    v, st, gamma, beta, _ = branch(case, mode, case_seed(case))
    if mutant in RECORD_MUTANTS:
        return elements_outside(records_model32(v, mutant), st["rec"], st["rec_bar"])[0]
    if mutant in TABLE_MUTANTS:
        a, d, _, _ = affine_model32(records_model32(v), gamma, beta, v.shape[1], mutant)
        tab = gn_tables_ref64(st, gamma, beta)
        return max(elements_outside(a, tab["a"], tab["a_bar"])[0], elements_outside(d, tab["d"], tab["d_bar"])[0])
    res = 2 if mutant == "main_table" else 1
    return elements_outside(*output_of(case, mode, res, 1, mutant))[0]


@pytest.mark.parametrize("mode", GEMM_MODES)
@pytest.mark.parametrize("mutant", RECORD_MUTANTS + TABLE_MUTANTS + OUTPUT_MUTANTS)
def test_mutants_leave_the_bars(mutant, mode):
    cases = mutant_cases(mutant, mode)
    if not cases:
        return                                                # (a pair cut off twice is 2^-16 |y| off: inside what its split is allowed)
    worst = {case: mutant_worst(mutant, mode, case) for case in cases}
    assert max(worst.values()) > 1.0, worst


def survey():
    m = measured_constants()
    print("measured constants (largest ratio of the honest model to the fp64 reference), per mode and over all:")
    for name in m:
        per = {mode: max(v for k, v in m[name].items() if k[0] == mode) for mode in GEMM_MODES}
        print(f"  {name}  " + "  ".join(f"{k} {v:.3f}" for k, v in per.items()) + f"   all {max(per.values()):.3f}")
    print("honest model, worst |err| / bar per mode: records / tables / output")
    for mode in GEMM_MODES:
        wr = wt = wo = 0.0
        for case in GNREC_CASES:
            v, st, gamma, beta, _ = branch(case, mode, case_seed(case))
            rec = records_model32(v)
            wr = max(wr, elements_outside(rec, st["rec"], st["rec_bar"])[0])
            a, d, _, _ = affine_model32(rec, gamma, beta, v.shape[1])
            tab = gn_tables_ref64(st, gamma, beta)
            wt = max(wt, elements_outside(a, tab["a"], tab["a_bar"])[0], elements_outside(d, tab["d"], tab["d_bar"])[0])
            for res in (0, 1, 2):
                wo = max(wo, elements_outside(*output_of(case, mode, res, 1))[0])
        print(f"  {mode:7s} {wr:.3f} / {wt:.3f} / {wo:.3f}")
    print("mutants, per mode: cases on which the mutant leaves its bar / cases it applies to, and the largest |err| / bar")
    for mutant in RECORD_MUTANTS + TABLE_MUTANTS + OUTPUT_MUTANTS:
        row = []
        for mode in GEMM_MODES:
            ws = [mutant_worst(mutant, mode, c) for c in mutant_cases(mutant, mode)]
            row.append(f"{mode} {sum(w > 1.0 for w in ws)}/{len(ws)} {max(ws) if ws else float('nan'):.3g}")
        print(f"  {mutant:16s} " + "   ".join(row))
    row = []
    for mode in GEMM_MODES:
        ws = [mutant_worst("var_fp32", mode, c) for c in GNREC_CASES]
        row.append(f"{mode} {sum(w > 1.0 for w in ws)}/{len(ws)} {max(ws):.3g}")
    print("  var_fp32 behind a convolution (not asserted): " + "   ".join(row))


if __name__ == "__main__":
    survey()
