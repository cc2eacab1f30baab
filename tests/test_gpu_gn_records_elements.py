"""The conv + GroupNorm record path and its fold, judged element by element against fp64: the records every kernel that calls
gn_records writes (csrc/gemm_impl.h: the tiled kernels' epilogue; csrc/conv1x1.hip: the streaming kernel's C1_PLAIN and
C1_STATS forms), the affines gn_affine_to_lds forms from them (csrc/norm.hip: gn_finalize_kernel's tables), and what
gn_apply_kernel and the C1_GN epilogue store -- with no shortcut, a plain one, and the downsample branch behind a GroupNorm of
its own.

tests/test_gpu_conv1x1_stream.py, tests/test_gpu_conv1x1_gn_epilogue.py and tests/test_gpu_ops.py compare these kernels with
one another bit for bit, and with references by one number per tensor or per group, on operands whose groups all look alike:
the code the kernels share, a record one block late, a neighbouring group's sums or a wrong d[c] in a small channel pass there.
Here every (image, group) has a mean, a sigma and a ratio r = |mean| / sigma of its own (tests/gpu_util.py conv_gn_operands; r
from 0 to 28: the one-pass variance cancels up to 1 + r^2 = 785 to 1), every output and every record is pre-filled with NaN
and sits behind guards, and every single record, table entry and output element is held to the bars of conv_gn_stats64,
gn_tables_ref64 and gn_records_out_ref64, whose constants tests/test_gn_records_bound_host.py measures on a CPU -- where it
also shows which mistakes the bars reject.  profiles/gn_records_elements.md has the figures."""
import functools

import pytest
import torch

from omnidata_amd.engine import DTYPES, load_library
from tests.gpu_util import (GEMM_PLANES, GNREC_CASES, SENTINEL, PlaneArena, assert_elements_inside, assert_r_coverage, conv_acc64,
                            conv_gn_geometry, conv_gn_operands, conv_gn_stats64, debug_flags, f32_guards_intact, gemm_elem_bound,
                            gemm_operand_planes, gn_map_operands, gn_records_out_ref64, gn_tables_ref64, guarded_f32, plane_value,
                            ptr, records_of, stats_of_records, stream)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
ONE_PLANE = ("bf16", "fp16")
TWO_PLANE = ("bf16x3", "fp16x3")
# the classes the plane modes are judged on: cpg 2 (1x1), a 3x3, cpg 32
PLANE_CASES = ((3, 8, 12, 64, 64, 1, 1), (3, 8, 12, 128, 128, 3, 1), (3, 8, 12, 256, 1024, 1, 1))
# what the streaming kernel can run (conv1x1_stream_eligible), and what the fold can (conv1x1_gn_eligible: stride 1)
STREAM_CASES = tuple(c for c in GNREC_CASES if c[5] == 1 and c[3] in (64, 128, 256))
FOLD_CASES = tuple(c for c in STREAM_CASES if c[6] == 1)
# The larger tile forms of launch_dt (csrc/gemm_impl.h) whose launch may carry records, on maps with rows per image % 32 == 0:
# (case, modes, debug flags whose results must agree bit for bit).  256x32 serves N = 32 only, where a group is one channel:
# launch_gemm refuses records there (gn_cpg < 2), so that form has no case.
TILE_CASES = {
    "256x256-pingpong": ((6, 96, 90, 256, 256, 3, 1), ONE_PLANE, (0,)),      # M = 51840: gemm_pp_kernel, the staged epilogue
    "256x64":           ((13, 96, 92, 64, 64, 3, 1), ONE_PLANE, (0,)),       # ceil(M / 256) = 449 >= 448
    "128x64":           ((7, 96, 92, 64, 64, 3, 1), ONE_PLANE + TWO_PLANE, (0,)),   # ceil(M / 128) = 483 >= 448 > ceil(M / 256)
    "128x128":          ((4, 96, 92, 128, 128, 3, 1), ONE_PLANE, (0,)),      # 276 tiles >= 256: four waves
    "128x128-8-waves":  ((4, 96, 92, 128, 128, 3, 1), TWO_PLANE, (0, 4)),    # 276 >= 200: gemm_pp2_kernel; flag 4: lockstep
}
# (B, HW, C) of the apply pass alone: 1, 3, 9 and 72 records (72: nine per slice of gn_affine_to_lds; 1, 3, 9: ragged slices);
# B = 32 at HW = 2304: C = 64 keeps one block per 256-pixel chunk (nch = 9 < want = 32), C = 256 has nb = want = 32 < nch = 36
# -- the fat-block partition, 72 pixels per block; C = 1024: four channels per thread of the affine loop
APPLY_CASES = ((2, 32, 64), (3, 96, 256), (2, 288, 64), (2, 96, 1024), (1, 2304, 64), (32, 2304, 64), (32, 2304, 256))


def case_seed(case):
    return case[3] + case[4] + 7 * case[5] + case[0]


class Launch:
    """The inputs and the guarded outputs of one test in `mode`.  One plane: every output a buffer of its own, NaN with guards.
    A pair: everything in one PlaneArena whose both planes are NaN wherever no input lies; after the launches whatever is not
    an output must hold the bits it held before.  fp32 outputs (records, tables): NaN with guards in either case."""

    def __init__(self, mode, elems):
        self.mode = mode
        self.dt, self.pl = GEMM_PLANES[mode]
        self.outs, self.bufs, self.f32 = [], [], []
        self.arena = None
        if self.pl == 2:
            self.arena = PlaneArena(elems + 64 * 4096, DEV, self.dt)
            self.arena.buf.view(torch.int16).fill_(SENTINEL)

    def put(self, t):
        return self.arena.put(t) if self.pl == 2 else t.float().to(self.dt).to(DEV).contiguous()

    def out(self, shape, guard):
        n = 1
        for s in shape:
            n *= s
        if self.pl == 2:
            self.arena.empty(guard)
            y = self.arena.empty(n)
            self.arena.empty(guard)
        else:
            buf = torch.full((n + 2 * guard,), SENTINEL, device=DEV, dtype=torch.int16)
            self.bufs.append((buf, n, guard))
            y = buf[guard:guard + n].view(self.dt)
        self.outs.append(y)
        return y.view(*shape)

    def copy(self, y, src):
        """an output that is an input as well (the in-place apply): the planes of src, bit for bit"""
        y.copy_(src)
        if self.pl == 2:
            self.arena.lo(y).copy_(self.arena.lo(src))

    def out_f32(self, shape, guard):
        n = 1
        for s in shape:
            n *= s
        buf, v = guarded_f32(n, guard)
        self.f32.append((buf, n, guard))
        return v.view(*shape)

    def arm(self):
        if self.pl == 2:
            self.before = self.arena.buf.clone()

    def check(self):
        """nothing but the outputs was written"""
        torch.cuda.synchronize()
        for buf, n, g in self.f32:
            assert f32_guards_intact(buf, n, g), "written outside an fp32 output"
        if self.pl == 2:
            keep = torch.ones(self.arena.total, dtype=torch.bool, device=DEV)
            for y in self.outs:
                o = (y.data_ptr() - self.arena.buf.data_ptr()) // 2
                keep[o:o + y.numel()] = False
            a, b = self.arena.buf.view(torch.int16), self.before.view(torch.int16)
            assert torch.equal(a[:, keep], b[:, keep]), "written outside the outputs"
        else:
            for buf, n, g in self.bufs:
                assert bool((buf[:g] == SENTINEL).all()) and bool((buf[g + n:] == SENTINEL).all()), "written outside an output"

    def value(self, y):
        """fp64 value (hi + lo) of a tensor of this launch, on the device"""
        return self.arena.value(y) if self.pl == 2 else y.double()

    def bits(self, y):
        b = y.view(torch.int16).clone()
        return torch.stack([b, self.arena.lo(y).view(torch.int16).clone()]) if self.pl == 2 else b

    def close(self):
        if self.arena is not None:
            self.arena.release()


@functools.lru_cache(maxsize=None)
def small_operands(case, seed):
    return conv_gn_operands(*case, seed)


@functools.lru_cache(maxsize=1)
def large_operands(case, seed):
    return conv_gn_operands(*case, seed)


def operands(case, seed):
    """the GNREC_CASES stay cached (a few MB each, shared by the tests); of the TILE_CASES only the one in use"""
    return small_operands(case, seed) if case in GNREC_CASES else large_operands(case, seed)


def reference(case, mode, seed):
    """(acc, S, statistics, tables) in fp64 on the device, from the values the kernel reads; asserts the case's r coverage"""
    pad, Ho, Wo = conv_gn_geometry(case)
    X, Wt, gamma, beta, _ = operands(case, seed)
    xv = plane_value(gemm_operand_planes(X, mode)).to(DEV)
    wv = plane_value(gemm_operand_planes(Wt, mode)).to(DEV)
    acc, S = conv_acc64(xv, wv, case[6], pad, pad, Ho, Wo)
    st = conv_gn_stats64(mode, acc, S, EPS)
    assert_r_coverage(st)
    return acc, S, st, gn_tables_ref64(st, gamma.float(), beta.float())


small_reference = functools.lru_cache(maxsize=None)(reference)   # the GNREC_CASES: a few MB each, shared by the tests


def elems_of(case):
    B, H, W, Cin, Cout, k, stride = case
    return B * H * W * Cin + Cout * k * k * Cin + 3 * B * (H // stride) * (W // stride) * Cout


class Conv:
    """one convolution of a case inside a Launch: its operands on the device and the outputs of dptx_op_conv_groupnorm"""

    def __init__(self, L, case, seed):
        self.L, self.case, self.seed = L, case, seed
        B, H, W, Cin, Cout, k, stride = case
        self.pad, self.Ho, self.Wo = conv_gn_geometry(case)
        self.HW = self.Ho * self.Wo
        X, Wt, gamma, beta, R = operands(case, seed)
        self.X, self.Wt, self.R = L.put(X), L.put(Wt), L.put(R)
        self.gamma, self.beta = gamma.float().to(DEV), beta.float().to(DEV)

    def outputs(self):
        B, Cout = self.case[0], self.case[4]
        raw = self.L.out((B, self.HW, Cout), self.Wo * Cout)
        Y = self.L.out((B, self.HW, Cout), self.Wo * Cout)
        rec = self.L.out_f32((B, self.HW // 32, 32, 2), 64 * 4)      # the guard behind it: four records past the last block
        return raw, Y, rec

    def run(self, flags, res, relu, raw, Y, rec):
        B, H, W, Cin, Cout, k, stride = self.case
        with debug_flags(flags):
            rc = load_library().dptx_op_conv_groupnorm(
                DTYPES[self.L.mode], ptr(self.X), ptr(self.Wt), ptr(raw), ptr(self.gamma), ptr(self.beta), ptr(self.R) if res else None,
                ptr(Y), B, H, W, Cin, Cout, k, stride, self.pad, self.pad, self.Ho, self.Wo, relu, EPS, ptr(rec), stream())
        assert rc == 0, (flags, rc)


def judge_records(rec, st, what):
    return assert_elements_inside(rec, st["rec"], st["rec_bar"], f"records {what}")


def judge_raw(L, raw, acc, S, what):
    y = acc.reshape(raw.shape)
    return assert_elements_inside(L.value(raw), y, gemm_elem_bound(L.mode, y, S.reshape(raw.shape), 0), f"raw map {what}")


def judge_output(L, Y, raw, tab, R, rtab, relu, what):
    y, bound = gn_records_out_ref64(L.mode, L.value(raw), tab, None if R is None else L.value(R), rtab, relu)
    return assert_elements_inside(L.value(Y).reshape(y.shape), y, bound, f"output {what}")


def op_records(L, X, gamma, beta, rec, R, r_gamma, r_beta, r_rec, Y, B, HW, C, relu):
    rc = load_library().dptx_op_groupnorm_records(DTYPES[L.mode], ptr(X), ptr(gamma), ptr(beta), ptr(rec), ptr(R), ptr(r_gamma),
                                                  ptr(r_beta), ptr(r_rec), ptr(Y), B, HW, C, relu, EPS, stream())
    assert rc == 0, rc


def same_bits(L, a, b):
    return torch.equal(L.bits(a), L.bits(b))


# ------------------------------------------------------------------------------------------- conv, then the apply pass
def unfused_case(mode, case, flag_list):
    """dptx_op_conv_groupnorm under every flag of flag_list: records, raw map and output of every launch inside their bars,
    all launches equal bit for bit; then dptx_op_groupnorm_records on the raw map and the records the convolution wrote: the
    same bits again, and the downsample form (the shortcut a second convolution's raw map behind its own GroupNorm, from
    that convolution's records) inside its bar"""
    seed = case_seed(case)
    B, Cout = case[0], case[4]
    acc, S, st, tab = small_reference(case, mode, seed)
    _, _, _, tab2 = small_reference(case, mode, seed + 1)
    L = Launch(mode, 2 * elems_of(case) + 12 * B * (case[1] // case[6]) * (case[2] // case[6]) * Cout)
    try:
        c1, c2 = Conv(L, case, seed), Conv(L, case, seed + 1)
        HW = c1.HW
        first = {}
        runs = [(f, res, relu) for f in flag_list for res, relu in (((0, 0), (0, 1), (1, 0), (1, 1)) if f == flag_list[0] else ((1, 1),))]
        outs = [c1.outputs() for _ in runs]
        raw2, Y2, rec2 = c2.outputs()
        new = [L.out((B, HW, Cout), Cout) for _ in range(3)]
        L.arm()
        for (f, res, relu), (raw, Y, rec) in zip(runs, outs):
            c1.run(f, res, relu, raw, Y, rec)
        c2.run(flag_list[0], 0, 0, raw2, Y2, rec2)
        raw, Y11, rec = outs[3]
        op_records(L, raw, c1.gamma, c1.beta, rec, None, None, None, None, new[0], B, HW, Cout, 1)
        op_records(L, raw, c1.gamma, c1.beta, rec, c1.R, None, None, None, new[1], B, HW, Cout, 1)
        op_records(L, raw, c1.gamma, c1.beta, rec, raw2, c2.gamma, c2.beta, rec2, new[2], B, HW, Cout, 1)
        L.check()
        for (f, res, relu), (raw_i, Y_i, rec_i) in zip(runs, outs):
            what = f"{mode} {case} flags {f} res {res} relu {relu}"
            judge_records(rec_i, st, what)
            judge_raw(L, raw_i, acc, S, what)
            judge_output(L, Y_i, raw_i, tab, c1.R if res else None, None, relu, what)
            first.setdefault((res, relu), (raw_i, Y_i, rec_i))
            r0, y0, q0 = first[(res, relu)]
            assert same_bits(L, raw_i, r0) and same_bits(L, Y_i, y0) and torch.equal(rec_i, q0), f"{what}: the kernels differ"
            assert torch.equal(rec_i, outs[0][2]) and same_bits(L, raw_i, outs[0][0]), what
        assert same_bits(L, new[0], outs[1][1]), "the new op differs from the apply pass of dptx_op_conv_groupnorm (no shortcut)"
        assert same_bits(L, new[1], Y11), "the new op differs from the apply pass of dptx_op_conv_groupnorm (plain shortcut)"
        judge_records(rec2, small_reference(case, mode, seed + 1)[2], f"{mode} {case} second branch")
        judge_output(L, new[2], raw, tab, raw2, tab2, 1, f"{mode} {case} new op, shortcut behind its own GroupNorm")
    finally:
        L.close()


@pytest.mark.parametrize("mode", ONE_PLANE)
@pytest.mark.parametrize("case", GNREC_CASES)
def test_conv_groupnorm_elements(case, mode):
    """flag 8: the tiled kernels (gn_records in the epilogue of gemm_impl.h); 0: the forward's dispatch; 16: the streaming
    kernel wherever it can run (C1_PLAIN with records)"""
    unfused_case(mode, case, (8, 0, 16))


@pytest.mark.parametrize("mode", TWO_PLANE)
@pytest.mark.parametrize("case", PLANE_CASES)
def test_conv_groupnorm_elements_planes(case, mode):
    unfused_case(mode, case, (0,))


# ---------------------------------------------------------------------------------------------------- the larger tile forms
@pytest.mark.parametrize("name,mode", [(n, m) for n in TILE_CASES for m in TILE_CASES[n][1]])
def test_records_of_the_larger_tiles(name, mode):
    case, _, flag_list = TILE_CASES[name]
    seed = case_seed(case)
    B, Cout = case[0], case[4]
    acc, S, st, tab = reference(case, mode, seed)
    L = Launch(mode, elems_of(case) + (2 * len(flag_list) + 1) * acc.numel())
    try:
        c = Conv(L, case, seed)
        outs = [c.outputs() for _ in flag_list]
        L.arm()
        for f, (raw, Y, rec) in zip(flag_list, outs):
            c.run(f, 1, 1, raw, Y, rec)
        L.check()
        for f, (raw, Y, rec) in zip(flag_list, outs):
            what = f"{name} {mode} flags {f}"
            judge_records(rec, st, what)
            judge_raw(L, raw, acc, S, what)
            judge_output(L, Y, raw, tab, c.R, None, 1, what)
            assert torch.equal(rec, outs[0][2]) and same_bits(L, Y, outs[0][1]), what
    finally:
        L.close()


# ------------------------------------------------------------------------------------------------------------- the fold
def run_fused(L, c, res, relu, passes, Y, rec, tab, c2=None, raw2=None, rec2=None):
    B, H, W, Cin, Cout, _, _ = c.case
    R = None if res == 0 else (c.R if res == 1 else raw2)
    rc = load_library().dptx_op_conv_groupnorm_fused(
        DTYPES[L.mode], ptr(c.X), ptr(c.Wt), ptr(c.gamma), ptr(c.beta), ptr(R), ptr(c2.gamma) if res == 2 else None,
        ptr(c2.beta) if res == 2 else None, ptr(rec2) if res == 2 else None, ptr(Y), B, H, W, Cin, Cout, relu, EPS, ptr(rec), ptr(tab),
        passes, stream())
    assert rc == 0, (res, relu, passes, rc)


def judge_tables(t, tab, rtab, what):
    """every entry of tables [B, 4, C]: rows 0 / 1 = (a, d); rows 2 / 3 = (ra, rd), or untouched without r_records"""
    assert_elements_inside(t[:, 0], tab["a"], tab["a_bar"], f"table a {what}")
    assert_elements_inside(t[:, 1], tab["d"], tab["d_bar"], f"table d {what}")
    if rtab is None:
        assert bool(torch.isnan(t[:, 2:]).all()), f"{what}: rows 2 / 3 written without r_records"
    else:
        assert_elements_inside(t[:, 2], rtab["a"], rtab["a_bar"], f"table ra {what}")
        assert_elements_inside(t[:, 3], rtab["d"], rtab["d_bar"], f"table rd {what}")


@pytest.mark.parametrize("mode", ONE_PLANE)
@pytest.mark.parametrize("case", FOLD_CASES)
def test_fold_elements(case, mode):
    """dptx_op_conv_groupnorm_fused: the statistics pass alone (passes = 1: C1_STATS; Y stays at its sentinel), statistics +
    finalize (3) and the whole op (7) with no shortcut, a plain one and the downsample form, ReLU off and on: every record,
    every table entry, every output element.  The new op with the downsample form must equal the fold bit for bit."""
    seed = case_seed(case)
    B, Cout = case[0], case[4]
    _, _, st, tab = small_reference(case, mode, seed)
    _, _, st2, tab2 = small_reference(case, mode, seed + 1)
    L = Launch(mode, 0)
    try:
        c1, c2 = Conv(L, case, seed), Conv(L, case, seed + 1)
        HW = c1.HW
        raw, Yu, recu = c1.outputs()
        raw2, Y2, rec2 = c2.outputs()
        mk = lambda: (L.out((B, HW, Cout), Cout), L.out_f32((B, HW // 32, 32, 2), 256), L.out_f32((B, 4, Cout), Cout))
        s1, s3, s3r = mk(), mk(), mk()
        full = {(res, relu): mk() for res in (0, 1, 2) for relu in (0, 1)}
        new = L.out((B, HW, Cout), Cout)
        L.arm()
        c1.run(8, 0, 0, raw, Yu, recu)                       # the raw map, which the fold never stores: the x of the reference
        c2.run(8, 0, 0, raw2, Y2, rec2)
        run_fused(L, c1, 0, 0, 1, *s1)
        run_fused(L, c1, 1, 1, 3, *s3)
        run_fused(L, c1, 2, 1, 3, *s3r, c2, raw2, rec2)
        for (res, relu), o in full.items():
            run_fused(L, c1, res, relu, 7, *o, c2, raw2, rec2)
        op_records(L, raw, c1.gamma, c1.beta, recu, raw2, c2.gamma, c2.beta, rec2, new, B, HW, Cout, 1)
        torch.cuda.synchronize()
        for o in (s1, s3, s3r):                              # no epilogue pass: Y untouched
            assert bool((o[0].view(torch.int16) == SENTINEL).all()), "a pass without the epilogue wrote Y"
        L.check()
        judge_records(rec2, st2, f"{mode} {case} second branch")
        judge_records(s1[1], st, f"{mode} {case} passes 1 (C1_STATS)")
        assert bool(torch.isnan(s1[2]).all()), "the statistics pass wrote the tables"
        for o, rt, what in ((s3, None, "passes 3"), (s3r, tab2, "passes 3 with r_records")):
            judge_records(o[1], st, f"{mode} {case} {what}")
            judge_tables(o[2], tab, rt, f"{mode} {case} {what}")
        for (res, relu), (Y, rec, t) in full.items():
            what = f"{mode} {case} passes 7 res {res} relu {relu}"
            judge_records(rec, st, what)
            judge_tables(t, tab, tab2 if res == 2 else None, what)
            judge_output(L, Y, raw, tab, None if res == 0 else (c1.R if res == 1 else raw2), tab2 if res == 2 else None, relu, what)
        assert torch.equal(new, full[(2, 1)][0]), "the new op's downsample form differs from the fold's"
    finally:
        L.close()


# -------------------------------------------------------------------------------- tables and the apply pass from exact records
@functools.lru_cache(maxsize=None)
def small_map_operands(shape):
    B, HW, C = shape
    return gn_map_operands(B, HW, C, seed=HW + C)


def map_operands(shape):
    """the batches of 32 (up to 150 MB a tensor) are not kept"""
    return small_map_operands(shape) if shape[0] <= 3 else gn_map_operands(*shape, seed=shape[1] + shape[2])


@pytest.mark.parametrize("mode", ONE_PLANE)
@pytest.mark.parametrize("shape", [s for s in APPLY_CASES if s[0] <= 3])
def test_tables_from_exact_records(shape, mode):
    """gn_finalize_kernel alone (passes = 2) on records computed in fp64 and rounded to fp32: only gn_affine_to_lds is under
    test, and the bar is that of its own roundings -- 2 u on a.  With r up to 28 this is where a variance formed in fp32
    (u (1 + r^2) = 785 u) shows; behind a convolution the accumulators' share of the bar hides it."""
    B, HW, C = shape
    x64, gamma, beta, _ = map_operands(shape)
    L = Launch(mode, 0)
    try:
        x = L.put(x64)
        x2 = L.put(x64.flip(0) * 0.5 + 1.0)
        rec, rec2 = records_of(L.value(x)).to(DEV), records_of(L.value(x2)).to(DEV)
        g, b = gamma.float().to(DEV), beta.float().to(DEV)
        g2, b2 = b.clone(), g.clone()
        tab = gn_tables_ref64(stats_of_records(rec, HW, C // 32, EPS), g, b)
        tab2 = gn_tables_ref64(stats_of_records(rec2, HW, C // 32, EPS), g2, b2)
        assert float(stats_of_records(rec, HW, C // 32, EPS)["r"].max()) >= 24.0
        w = L.put(torch.zeros(C, 1, 1, 64))
        Y = L.out((B, HW, C), C)
        t1, t2 = L.out_f32((B, 4, C), C), L.out_f32((B, 4, C), C)
        L.arm()
        lib = load_library()
        for t, r_args in ((t1, (None, None, None, None)), (t2, (ptr(x2), ptr(g2), ptr(b2), ptr(rec2)))):
            rc = lib.dptx_op_conv_groupnorm_fused(DTYPES[mode], ptr(x), ptr(w), ptr(g), ptr(b), *r_args, ptr(Y), B, HW, 1, 64, C, 1, EPS,
                                                  ptr(rec), ptr(t), 2, stream())
            assert rc == 0, rc
        L.check()
        assert bool((Y.view(torch.int16) == SENTINEL).all())
        judge_tables(t1, tab, None, f"{mode} {shape} finalize from exact records")
        judge_tables(t2, tab, tab2, f"{mode} {shape} finalize from exact records, with r_records")
    finally:
        L.close()


@pytest.mark.parametrize("mode", ONE_PLANE + TWO_PLANE)
@pytest.mark.parametrize("shape", APPLY_CASES)
def test_apply_pass_from_exact_records(shape, mode):
    """dptx_op_groupnorm_records on records computed in fp64 and rounded to fp32: only gn_apply_kernel is under test.  No
    shortcut, a plain one and one behind its own GroupNorm (the batches of 32: the plain one); in place (Y == X, how the
    forward calls it) equals out of place, and image 1 of a batch equals that image alone, bit for bit."""
    B, HW, C = shape
    x64, gamma, beta, R64 = map_operands(shape)
    forms = (1,) if B > 3 else (0, 1, 2)
    L = Launch(mode, (5 + len(forms)) * x64.numel())
    try:
        x, R = L.put(x64), L.put(R64)
        rec, rrec = records_of(L.value(x)).to(DEV), records_of(L.value(R)).to(DEV)
        g, b = gamma.float().to(DEV), beta.float().to(DEV)
        g2, b2 = b.clone(), g.clone()
        tab = gn_tables_ref64(stats_of_records(rec, HW, C // 32, EPS), g, b)
        rtab = gn_tables_ref64(stats_of_records(rrec, HW, C // 32, EPS), g2, b2)
        outs = [L.out((B, HW, C), C) for _ in forms]
        inplace = L.out((B, HW, C), C)
        one = L.out((1, HW, C), C)
        L.copy(inplace, x)
        L.arm()
        args = {0: (None, None, None, None), 1: (R, None, None, None), 2: (R, g2, b2, rrec)}
        for f, Y in zip(forms, outs):
            op_records(L, x, g, b, rec, *args[f], Y, B, HW, C, 1)
        op_records(L, inplace, g, b, rec, *args[forms[-1]], inplace, B, HW, C, 1)
        i = min(1, B - 1)
        sub = lambda t: None if t is None or t.dim() < 3 else t[i:i + 1]
        a1 = args[forms[-1]]
        op_records(L, x[i:i + 1], g, b, rec[i:i + 1], sub(a1[0]), a1[1], a1[2], None if a1[3] is None else a1[3][i:i + 1], one, 1, HW, C, 1)
        L.check()
        for f, Y in zip(forms, outs):
            judge_output(L, Y, x, tab, None if f == 0 else R, rtab if f == 2 else None, 1, f"apply alone {mode} {shape} shortcut form {f}")
        assert same_bits(L, inplace, outs[-1]), "in place differs from out of place"
        assert same_bits(L, one, outs[-1][i:i + 1]), "image 1 of the batch differs from that image alone"
    finally:
        L.close()


def test_the_new_op_refuses_what_it_cannot_run():
    lib = load_library()
    x = torch.zeros(1, 96, 64, device=DEV, dtype=torch.bfloat16)
    f = torch.zeros(4096, device=DEV)
    call = lambda HW, R, rg, rb, rr: lib.dptx_op_groupnorm_records(DTYPES["bf16"], ptr(x), ptr(f), ptr(f), ptr(f), R, rg, rb, rr, ptr(x), 1,
                                                                    HW, 64, 0, EPS, stream())
    assert call(96, None, None, None, None) == 0
    assert call(80, None, None, None, None) != 0                         # HW % 32 != 0
    assert call(96, ptr(x), ptr(f), None, None) != 0                     # r_gamma without r_beta and r_records
    assert call(96, ptr(x), ptr(f), ptr(f), None) != 0
    assert call(96, None, ptr(f), ptr(f), ptr(f)) != 0                   # without R
    torch.cuda.synchronize()
