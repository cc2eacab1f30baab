"""The implicit-GEMM kernels (csrc/gemm_impl.h, gemm*.hip, conv1x1.hip) judged element by element against fp64.

Every output element of every case must lie within tests/gpu_util.gemm_elem_bound of the fp64 value of the expression on the
values the kernel actually reads (one 16-bit plane, hi + lo, or the hi plane alone where a form reads only that):
u |y| + F S for a 16-bit output, F S for an fp32 one, (3 u^2 + F) S for a hi / lo pair.  The operands carry a scale of their
own in every row and column (scaled_gemm_operands / scaled_conv_operands), so a small row next to a large one is judged by its
own size; the maps are rectangular, pad_t != pad_l occurs, and every branch of launch_dt is reached.  What the bound is worth --
which mistakes it rejects -- is shown on a CPU in tests/test_gemm_bound_host.py; profiles/gemm_elements.md has the worst
|err| / bound of every case.  Outputs start as NaN and carry one guard row behind the last: an element that is not written, or
a row written past M, fails.  pytest -m gpu."""
import pytest
import torch

from omnidata_amd.engine import DTYPES, load_library
from tests.gpu_util import (GEMM_MODES, GEMM_PLANES, PlaneArena, assert_elements_inside, conv_acc64, epilogue_ref64, gemm_elem_bound,
                            gemm_ref64, ptr, scaled_conv_operands, scaled_gemm_operands, stream)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


class Arena(PlaneArena):
    """PlaneArena in every mode: the one-plane modes read and write the hi plane, and their values are that plane's."""

    def __init__(self, mode, elems):
        dt, self.pl = GEMM_PLANES[mode]
        super().__init__(elems + 8192, dtype=dt)

    def val(self, t, planes=None):
        """fp64 value of what a kernel reads from / wrote to t: hi + lo, or hi alone (planes = 1)"""
        return self.value(t) if (self.pl if planes is None else planes) == 2 else t.double()

    def out(self, M, N):
        """[M + 1, N] output: M rows for the kernel and one guard row"""
        return self.empty(M + 1, N)

    def fresh(self, full):
        full.fill_(NAN)
        self.lo(full).fill_(NAN)

    def bits(self, full, M):
        """copies of the planes of the first M rows, and the guard row's check"""
        assert torch.isnan(full[M].float()).all() and torch.isnan(self.lo(full)[M].float()).all(), "row M was written"
        return full[:M].clone(), self.lo(full)[:M].clone()


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int16), y.view(torch.int16)) if x.dtype != torch.float32 else
               torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


class gemm_flags:
    def __init__(self, flags):
        self.flags = flags

    def __enter__(self):
        assert load_library().dptx_debug_set_gemm_flags(self.flags) == 0

    def __exit__(self, *exc):
        load_library().dptx_debug_set_gemm_flags(0)


# ------------------------------------------------------------------------------------------------------------- dense GEMM
# (M, N, K, the tile launch_dt takes in the one-plane modes / in the plane modes)
GEMM_SHAPES = [
    (77, 192, 64, "64x64"),             # N % 128 != 0, 3 n-tiles of 64: the last branch; one k-tile, one full m-tile + 13 rows
    (57400, 64, 64, "128x64"),          # ceil(M / 128) = 449 >= 448, ceil(M / 256) = 225 < 448
    (114700, 64, 64, "256x64/128x64"),  # ceil(M / 256) = 449 >= 448: the 256x64 tile (one-plane modes only; plane modes 128x64)
    (300, 32, 1152, "256x32"),          # N == 32
    (5413, 768, 192, "128x128"),        # K < 512: no 256x256; 43 x 6 = 258 >= 256 tiles: 4 waves, 8 waves in the plane modes (>= 200)
    (17153, 768, 512, "256x256pp/128x128"),  # 68 x 3 = 204 >= 200 tiles, fill 0.80 x 1.5 >= 0.79: the ping-pong kernel; the last
                                             # m-tile holds one row; bias + R takes its register-direct residual form (res == 1)
]
# name -> (bias, act, residual: None / "16" / "32", c_fp32, a_fp32)
GEMM_EPILOGUES = {"plain": (0, 0, None, 0, 0), "bias+relu": (1, 1, None, 0, 0), "bias+gelu": (1, 2, None, 0, 0),
                  "bias+R16": (1, 0, "16", 0, 0), "bias+R32->fp32": (1, 0, "32", 1, 0), "A32+bias": (1, 0, None, 0, 1)}


@pytest.mark.parametrize("mode", GEMM_MODES)
@pytest.mark.parametrize("M,N,K,tile", GEMM_SHAPES, ids=[s[3].split("/")[0] for s in GEMM_SHAPES])
def test_gemm_elements(mode, M, N, K, tile):
    """dptx_op_gemm on one shape per branch of launch_dt, every epilogue that exists for the mode; on the 256x256 shape the
    staged epilogue (debug flag 1) and the one-block-per-tile launch (flag 3) must give the bits of flag 0."""
    lib = load_library()
    dt, pl = GEMM_PLANES[mode]
    A64, W64, b64, R64 = scaled_gemm_operands(M, N, K, seed=N + K)
    ar = Arena(mode, M * K + N * K + (2 * M + 1) * N)
    try:
        A, W, R, full = ar.put(A64), ar.put(W64), ar.put(R64), ar.out(M, N)
        bias, R32, A32 = b64.float().to(DEV), R64.float().to(DEV), A64.float().to(DEV)
        C32 = torch.empty(M + 1, N, device=DEV)
        del A64, W64, R64
        for name, (has_bias, act, res, c_fp32, a_fp32) in GEMM_EPILOGUES.items():
            # fp32 A is staged through registers: one-plane modes, and no 256-row tile (launch_cfg refuses both)
            if a_fp32 and (pl == 2 or tile.startswith(("256x32", "256x64"))):
                continue
            Rin = None if res is None else R if res == "16" else R32
            outs = []
            for flags in ((0, 1, 3) if tile.startswith("256x256") else (0,)):
                ar.fresh(full)
                C32.fill_(NAN)
                with gemm_flags(flags):
                    rc = lib.dptx_op_gemm(DTYPES[mode], ptr(A32 if a_fp32 else A), ptr(W), ptr(bias) if has_bias else None, ptr(Rin),
                                          ptr(C32 if c_fp32 else full), M, N, K, act, a_fp32, c_fp32, int(res == "32"), stream())
                assert rc == 0, (name, flags, rc)
                if c_fp32:
                    assert torch.isnan(C32[M]).all(), "row M was written"
                    outs.append((C32[:M].clone(),))
                else:
                    outs.append(ar.bits(full, M))
            for o in outs[1:]:
                assert same_bits(o, outs[0]), (name, "debug flags 1 / 3 change the bits")
            got = outs[0][0].double() if c_fp32 or pl == 1 else outs[0][0].double() + outs[0][1].double()
            Av = A32.to(dt).double() if a_fp32 else ar.val(A)
            Rv = None if res is None else ar.val(R) if res == "16" else R32.double()
            y, S = gemm_ref64(Av, ar.val(W), bias if has_bias else None, Rv, act)
            assert_elements_inside(got, y, gemm_elem_bound(mode, y, S, act, c_fp32=bool(c_fp32)),
                                   f"gemm {mode} ({M}, {N}, {K}) {tile} {name}")
    finally:
        ar.release()


# ------------------------------------------------------------------------------------------------------------ convolution
# geometry (B, H, W, Cin, Cout, k, stride, pad_t, pad_l, Ho, Wo); variants (a_relu, act, residual) per kind of mode (None: the
# case does not exist there); debug flags whose results must agree bit for bit, per kind of mode
V_PLAIN, V_RES = (0, 0, False), (0, 0, True)
CONV_CASES = {
    "rect-3x3":     ((3, 10, 14, 64, 64, 3, 1, 1, 1, 10, 14), [V_PLAIN, V_RES], [V_PLAIN, V_RES], (0,), (0,)),   # 140 rows per image: tiles straddle images
    "padt1-padl0":  ((2, 9, 14, 128, 128, 3, 2, 1, 0, 5, 7), [V_PLAIN, V_RES], [V_PLAIN, V_RES], (0,), (0,)),    # pad_t != pad_l, odd Wo
    "padt0-padl1":  ((2, 14, 9, 128, 128, 3, 2, 0, 1, 7, 5), [V_PLAIN, V_RES], [V_PLAIN, V_RES], (0,), (0,)),    # its transpose
    # strided 1x1 on odd sizes: flag 16 takes the streaming kernel (conv1x1.hip), 0 and 8 the tiled ones
    "1x1-stride2":  ((3, 9, 13, 256, 512, 1, 2, 0, 0, 5, 7), [V_PLAIN, (0, 1, False)], [V_PLAIN], (0, 8, 16), (0,)),
    "tap-fastest":  ((1, 6, 10, 512, 256, 3, 1, 1, 1, 6, 10), [(1, 0, False)], [(1, 0, False)], (0,), (0,)),     # Cin >= 512: k_tap_fast, a_relu
    "N32-relu":     ((1, 5, 9, 128, 32, 3, 1, 1, 1, 5, 9), [(0, 1, False)], [(0, 1, False)], (0,), (0,)),        # the 256x32 tile
    # M = 51840 = 202.5 x 256: 256x256 ping-pong (direct, a_relu and residual forms) with padding taps and a ragged last tile;
    # plane modes: the two-plane 128x128 ping-pong kernel (gemm_pp2_kernel), flag 4 = the lockstep kernel
    "pingpong":     ((6, 96, 90, 256, 256, 3, 1, 1, 1, 96, 90), [V_PLAIN, (1, 0, False), V_RES], [(0, 1, True)], (0,), (0, 4)),
    # M = 114816: ceil(M / 256) = 449 >= 448, the 256x64 tile (one-plane modes only)
    "256x64":       ((13, 96, 92, 64, 64, 3, 1, 1, 1, 96, 92), [V_PLAIN, V_RES], None, (0,), (0,)),
}
CONV_PARAMS = [(c, m) for c in CONV_CASES for m in GEMM_MODES if CONV_CASES[c][1 + (GEMM_PLANES[m][1] == 2)] is not None]


class ConvCase:
    """operands of one convolution case in an arena, and the fp64 accumulations of the values a form reads (cached)"""

    def __init__(self, mode, geo, seed):
        self.mode, self.geo = mode, geo
        B, H, W, Cin, Cout, k, stride, pad_t, pad_l, Ho, Wo = geo
        X64, W64, b64, R64 = scaled_conv_operands(B, H, W, Cin, Cout, k, seed, Ho, Wo)
        self.M = B * Ho * Wo
        self.ar = ar = Arena(mode, X64.numel() + W64.numel() + (2 * self.M + 1) * Cout)
        self.X, self.Wt, self.R, self.full = ar.put(X64), ar.put(W64), ar.put(R64), ar.out(self.M, Cout)
        self.bias = b64.float().to(DEV)
        self.acc = {}

    def ref(self, a_relu, act, res, x_planes=None, w_planes=None, r_planes=None):
        """(y, S) in fp64; *_planes = 1: the form reads the hi plane of that operand only"""
        B, H, W, Cin, Cout, k, stride, pad_t, pad_l, Ho, Wo = self.geo
        key = (a_relu, x_planes, w_planes)
        if key not in self.acc:
            self.acc[key] = conv_acc64(self.ar.val(self.X, x_planes), self.ar.val(self.Wt, w_planes), stride, pad_t, pad_l, Ho, Wo, a_relu)
        return epilogue_ref64(*self.acc[key], self.bias, self.ar.val(self.R, r_planes) if res else None, act)

    def got(self, bits, planes):
        B, _, _, _, Cout, _, _, _, _, Ho, Wo = self.geo
        v = bits[0].double() + bits[1].double() if planes == 2 else bits[0].double()
        return v.view(B, Ho, Wo, Cout)


@pytest.mark.parametrize("case,mode", CONV_PARAMS)
def test_conv_elements(case, mode):
    """dptx_op_conv on rectangular maps, pad_t != pad_l, odd output sizes, the tap-fastest k order, and the N = 32, 256x64,
    256x256 ping-pong and two-plane ping-pong kernels; where several kernels serve a case they must agree bit for bit."""
    lib = load_library()
    geo, v1, v2, f1, f2 = CONV_CASES[case]
    pl = GEMM_PLANES[mode][1]
    B, H, W, Cin, Cout, k, stride, pad_t, pad_l, Ho, Wo = geo
    c = ConvCase(mode, geo, seed=H + W)
    try:
        for a_relu, act, res in (v2 if pl == 2 else v1):
            outs = []
            for flags in (f2 if pl == 2 else f1):
                c.ar.fresh(c.full)
                with gemm_flags(flags):
                    rc = lib.dptx_op_conv(DTYPES[mode], ptr(c.X), ptr(c.Wt), ptr(c.bias), ptr(c.R) if res else None, ptr(c.full), B, H, W,
                                          Cin, Cout, k, stride, pad_t, pad_l, Ho, Wo, a_relu, act, stream())
                assert rc == 0, (flags, rc)
                outs.append(c.ar.bits(c.full, c.M))
            for o in outs[1:]:
                assert same_bits(o, outs[0]), "the kernels that serve this case differ"
            y, S = c.ref(a_relu, act, res)
            assert_elements_inside(c.got(outs[0], pl), y, gemm_elem_bound(mode, y, S, act),
                                   f"conv {mode} {case} a_relu={a_relu} act={act} res={int(res)}")
    finally:
        c.ar.release()


# --------------------------------------------------------------------------------------------- per-layer precision forms
# form -> (mode, epi2 argument of dptx_op_conv_planes, planes of X and of W the product reads)
PLANE_FORMS = {"fp16-hixhi-pair-epilogue": ("fp16", 1, 1, 1), "fp16x3-two-mfma": ("fp16x3", 2, 1, 2)}


@pytest.mark.parametrize("form", list(PLANE_FORMS))
@pytest.mark.parametrize("case", ["rect-3x3", "padt1-padl0", "padt0-padl1"])
def test_conv_plane_forms_elements(case, form):
    """dptx_op_conv_planes: epi2 = 1 (fp16: hi x hi product, two-plane R and Y) and epi2 = 2 (fp16x3: the hi plane of X only,
    its lo plane is NaN), each also with c_hi_only (the lo plane of Y stays untouched) and r1_hi_only, against fp64 of exactly
    the planes read."""
    lib = load_library()
    mode, epi2, xp, wp = PLANE_FORMS[form]
    geo = CONV_CASES[case][0]
    B, H, W, Cin, Cout, k, stride, pad_t, pad_l, Ho, Wo = geo
    c = ConvCase(mode, geo, seed=H + W)
    try:
        if epi2 == 2:
            c.ar.lo(c.X).fill_(NAN)
        for c_hi_only, r1_hi_only in ((0, 0), (1, 0), (0, 1)):
            c.ar.fresh(c.full)
            rc = lib.dptx_op_conv_planes(DTYPES[mode], ptr(c.X), ptr(c.Wt), ptr(c.bias), ptr(c.R), ptr(c.full), B, H, W, Cin, Cout, k,
                                         stride, pad_t, pad_l, Ho, Wo, 0, 0, epi2, c_hi_only, r1_hi_only, stream())
            assert rc == 0, rc
            planes = 1 if c_hi_only else 2
            if c_hi_only:
                assert torch.isnan(c.ar.lo(c.full).float()).all(), "c_hi_only wrote the lo plane"
                bits = (c.full[:c.M].clone(), None)
                assert torch.isnan(c.full[c.M].float()).all(), "row M was written"
            else:
                bits = c.ar.bits(c.full, c.M)
            y, S = c.ref(0, 0, True, x_planes=xp, w_planes=wp, r_planes=1 if r1_hi_only else 2)
            assert_elements_inside(c.got(bits, planes), y, gemm_elem_bound(mode, y, S, 0, planes=planes),
                                   f"conv_planes {form} {case} c_hi_only={c_hi_only} r1_hi_only={r1_hi_only}")
    finally:
        c.ar.release()
