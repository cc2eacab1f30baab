"""The glue kernels of csrc/misc.hip that ran only inside whole forwards, one launch each through their op entry points:
patchify16, depth_to_space, cast_f32, to_f32, amax, nonfinite_scan (exact: bit for bit against torch indexing and torch's own
roundings), readout_cls and pos_resize (every element against fp64).  Every output is pre-filled with NaN and sits behind
guard elements; one case of every kernel that caps its grid is large enough for the second trip of its grid-stride loop.
Every Inf / NaN below is an input bit pattern to a conversion or to an integer scan; the refusals are tested at the entry
point, which returns before any launch.  profiles/stem_elements.md has the figures."""
import pytest
import torch

from omnidata_amd.engine import DTYPES, load_library
from tests.gpu_util import (GEMM_F32_FLOOR_FACTOR, GEMM_F32_FLOOR_MEASURED, GEMM_MODES, GEMM_PLANES, POS_GRIDS, PlaneArena, Target,
                            assert_elements_inside, f32_guards_intact, gemm_ref64, guarded_f32, pos_elem_bound, pos_resize_ref64,
                            ptr, scaled_gemm_operands, scaled_pos_embed, stream)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IO = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}
ONE_PLANE = ("bf16", "fp16")
E_INVALID = -1


def lib():
    return load_library()


def test_invalid_code_is_the_headers():
    from tests.test_abi import header_text
    import re
    assert int(re.search(r"DPTX_E_INVALID\s*=\s*(-?\d+)", header_text()).group(1)) == E_INVALID


def scaled_values(n, seed, device=DEV):
    """n fp32 values N(0, 1) 2^((7 i mod 13) - 6) on the device"""
    g = torch.Generator(device=device).manual_seed(seed)
    i = torch.arange(n, device=device)
    return torch.randn(n, generator=g, device=device) * torch.exp2(((7 * i) % 13 - 6).float())


def split(v, mode):
    """(hi, lo) planes of fp32 values v as PlaneArena.put splits them, on v's device; lo None for one plane"""
    dt, pl = GEMM_PLANES[mode]
    hi = v.to(dt)
    return hi, ((v - hi.float()).to(dt) if pl == 2 else None)


def assert_same_bits(got, want, what):
    """equal bit for bit, a NaN judged as a NaN whatever its payload; on failure the first differing (index, got, want) bits"""
    got, want = got.flatten(), want.flatten()
    ib = torch.int32 if got.dtype == torch.float32 else torch.int16
    gn, wn = torch.isnan(got), torch.isnan(want)
    differ = (gn != wn) | (~gn & ~wn & (got.view(ib) != want.view(ib)))
    if bool(differ.any()):
        i = torch.nonzero(differ).flatten()[:5]
        first = [(int(j), hex(int(got.view(ib)[j]) & 0xFFFFFFFF), hex(int(want.view(ib)[j]) & 0xFFFFFFFF)) for j in i]
        raise AssertionError(f"{what}: {int(differ.sum())} of {got.numel()} elements differ, first (index, got, want) {first}")


def assert_planes(t, want_hi, want_lo):
    hi, lo = t.planes()
    assert_same_bits(hi, want_hi, "hi plane")
    if lo is not None:
        assert_same_bits(lo, want_lo, "lo plane")


# ------------------------------------------------------------------------------------------------------------------ patchify16
PATCH_CASES = [(1, 16, 16), (2, 32, 48), (3, 16, 80)]


def run_patchify(mode, io, case):
    B, H, W = case
    x = scaled_values(B * 3 * H * W, 11 + H + W).to(IO[io][1]).view(B, 3, H, W)
    n = B * (H // 16) * (W // 16) * 768
    t = Target(mode, n, 768)
    try:
        P = t.out()
        assert lib().dptx_op_patchify16(DTYPES[mode], ptr(x), IO[io][0], ptr(P), B, H, W, stream()) == 0
        want = x.float().view(B, 3, H // 16, 16, W // 16, 16).permute(0, 2, 4, 1, 3, 5).reshape(-1, 768)   # k = (c, ky, kx)
        assert_planes(t, *split(want, mode))
    finally:
        t.close()


@pytest.mark.parametrize("mode", GEMM_MODES)
@pytest.mark.parametrize("io", list(IO))
@pytest.mark.parametrize("case", PATCH_CASES)
def test_patchify16(mode, io, case):
    run_patchify(mode, io, case)


def test_patchify16_past_the_grid_cap():
    """19 x 48 x 48 patches x 96 vectors = 4 202 496 work items > 16384 x 256: the last 8192 come from the loop's second trip"""
    assert 19 * 48 * 48 * 96 > 16384 * 256
    run_patchify("bf16", "fp32", (19, 768, 768))


def test_patchify16_refusals():
    x = torch.zeros(3 * 32 * 32, device=DEV)
    buf, P = guarded_f32(768, 64)
    for args in ((DTYPES["bf16"], ptr(x), 0, ptr(P), 1, 24, 32), (DTYPES["bf16"], ptr(x), 0, ptr(P), 1, 32, 8),
                 (DTYPES["bf16"], ptr(x), 3, ptr(P), 1, 32, 32), (DTYPES["bf16"], ptr(x), 0, ptr(P), 0, 32, 32),
                 (7, ptr(x), 0, ptr(P), 1, 32, 32), (DTYPES["bf16"], None, 0, ptr(P), 1, 32, 32)):
        assert lib().dptx_op_patchify16(*args, stream()) == E_INVALID, args
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


# -------------------------------------------------------------------------------------------------------------- depth_to_space
D2S_CASES = [(1, 1, 1, 2, 8), (2, 3, 5, 4, 256), (2, 6, 4, 2, 512), (1, 2, 3, 3, 64)]


def run_d2s(mode, case):
    B, h, w, k, C = case
    n = B * h * w * k * k * C
    t = Target(mode, n, k * C, n)
    try:
        g = torch.Generator(device=DEV).manual_seed(n % 1000)
        bits = [torch.randint(-32768, 32767, (n,), generator=g, device=DEV, dtype=torch.int16) for _ in range(t.pl)]
        if t.pl == 2:
            G = t.arena.empty(n)
            G.view(torch.int16).copy_(bits[0])
            t.arena.lo(G).view(torch.int16).copy_(bits[1])
        else:
            G = bits[0].view(t.dt)
        Y = t.out()
        assert lib().dptx_op_depth_to_space(DTYPES[mode], ptr(G), ptr(Y), B, h, w, k, C, stream()) == 0
        hi, lo = t.planes()
        for got, src in zip((hi, lo)[:t.pl], bits):
            want = src.view(B, h, w, k, k, C).permute(0, 1, 3, 2, 4, 5).reshape(-1)     # Y[b][y k + dy][x k + dx][c]
            assert torch.equal(got.view(torch.int16).flatten(), want)
    finally:
        t.close()


@pytest.mark.parametrize("mode", GEMM_MODES)
@pytest.mark.parametrize("case", D2S_CASES)
def test_depth_to_space(mode, case):
    run_d2s(mode, case)


def test_depth_to_space_past_the_grid_cap():
    assert 8 * 24 * 24 * 16 * 64 > 16384 * 256
    run_d2s("bf16x3", (8, 24, 24, 4, 512))


def test_depth_to_space_refusals():
    buf, Y = guarded_f32(1024, 64)
    G = torch.zeros(2048, device=DEV)
    for args in ((DTYPES["bf16"], ptr(G), ptr(Y), 1, 2, 2, 2, 12), (DTYPES["bf16"], ptr(G), ptr(Y), 1, 2, 2, 0, 8),
                 (DTYPES["bf16"], ptr(G), ptr(Y), 0, 2, 2, 2, 8), (DTYPES["bf16"], ptr(G), ptr(G), 1, 2, 2, 2, 8),
                 (4, ptr(G), ptr(Y), 1, 2, 2, 2, 8)):
        assert lib().dptx_op_depth_to_space(*args, stream()) == E_INVALID, args
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


# ---------------------------------------------------------------------------------------------------------- cast_f32 and to_f32
def special_values(mode):
    """fp32 inputs (device) at which a conversion goes wrong: exact ties of the plane type (the midpoints above 4096 random
    16-bit numbers), values below 2^-14 and below 2^-24, +-0, 65504, 65520, -65520, +-Inf and NaN"""
    dt = GEMM_PLANES[mode][0]
    g = torch.Generator(device=DEV).manual_seed(5)
    h = (torch.randn(4096, generator=g, device=DEV) * torch.exp2(torch.arange(4096, device=DEV) % 24 - 12.0)).to(dt).float()
    ties = (h.view(torch.int32) | (0x8000 if dt == torch.bfloat16 else 0x1000)).view(torch.float32)
    assert bool((ties.to(dt).float() != ties).all())
    small = torch.tensor([2.0 ** -14, 1.3 * 2.0 ** -15, -1.7 * 2.0 ** -17, 2.0 ** -24, 1.5 * 2.0 ** -25, 1.1 * 2.0 ** -25, 2.0 ** -25,
                          -0.9 * 2.0 ** -25, 2.0 ** -26, 3.0 * 2.0 ** -24, 2.5 * 2.0 ** -24, 0.0, -0.0, 65504.0, 65520.0, -65520.0,
                          65519.996, float("inf"), float("-inf"), float("nan"), 1.0, -1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -8],
                         device=DEV)
    return torch.cat([ties, small])


@pytest.mark.parametrize("mode", GEMM_MODES)
@pytest.mark.parametrize("n", [4120 + 8 * 1000, 8192 * 256 * 8 + 8 * 1000])
def test_cast_f32(mode, n):
    """hi = rn(x), lo = rn(x - hi), bit for bit against torch's conversions (PlaneArena.put's split); the larger n is past the
    8192 x 256 x 8 elements of one trip of the kernel's grid-stride loop, and the special values sit at its very end too"""
    sp = special_values(mode)
    assert sp.numel() == 4120
    v = scaled_values(n, 21)
    v[:sp.numel()] = sp
    v[-sp.numel():] = sp.flip(0)
    t = Target(mode, n, 64)
    try:
        dst = t.out()
        assert lib().dptx_op_cast_f32(DTYPES[mode], ptr(v), ptr(dst), n, stream()) == 0
        assert_planes(t, *split(v, mode))
    finally:
        t.close()


@pytest.mark.parametrize("mode", GEMM_MODES)
@pytest.mark.parametrize("n", [4120 + 8 * 1000, 8192 * 256 * 8 + 8 * 1000])
def test_to_f32(mode, n):
    """dst = hi, or fl32(hi + lo) of a pair, bit for bit (a NaN judged as a NaN); the planes are torch's split of the values of
    test_cast_f32, so +-Inf (lo = NaN), the 65520 that rounds to Inf (lo = -Inf) and subnormal planes are among them"""
    sp = special_values(mode)
    v = scaled_values(n, 22)
    v[:sp.numel()] = sp
    v[-sp.numel():] = sp.flip(0)
    hi, lo = split(v, mode)
    dt, pl = GEMM_PLANES[mode]
    arena = None
    try:
        if pl == 2:
            arena = PlaneArena(n + 4096, DEV, dt)
            src = arena.empty(n)
            src.copy_(hi)
            arena.lo(src).copy_(lo)
        else:
            src = hi
        buf, dst = guarded_f32(n, 64)
        assert lib().dptx_op_to_f32(DTYPES[mode], ptr(src), ptr(dst), n, stream()) == 0
        torch.cuda.synchronize()
        assert f32_guards_intact(buf, n, 64)
        assert_same_bits(dst, hi.float() + lo.float() if pl == 2 else hi.float(), f"to_f32 {mode}")
    finally:
        if arena is not None:
            arena.release()


@pytest.mark.parametrize("n", [0, 4, 12, 8 * 100 + 1, -8])
def test_cast_and_to_f32_refuse_n_not_a_multiple_of_8(n):
    src = torch.ones(1024, device=DEV)
    src16 = torch.ones(1024, device=DEV, dtype=torch.bfloat16)
    buf, dst = guarded_f32(1024, 64)
    assert lib().dptx_op_cast_f32(DTYPES["bf16"], ptr(src), ptr(dst), n, stream()) == E_INVALID
    assert lib().dptx_op_to_f32(DTYPES["bf16"], ptr(src16), ptr(dst), n, stream()) == E_INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


# ------------------------------------------------------------------------------------------------------------------------ amax
def amax_of(mode, x, relu, initial=0):
    out = torch.tensor([initial], device=DEV, dtype=torch.int32)
    assert lib().dptx_op_amax(DTYPES[mode], ptr(x), x.numel(), relu, ptr(out), stream()) == 0
    torch.cuda.synchronize()
    return int(out.item())


def f32_bits(v):
    return int(torch.tensor([v], dtype=torch.float32).view(torch.int32).item())


@pytest.mark.parametrize("mode", ONE_PLANE)
def test_amax_places(mode):
    """*amax_bits is the bits of the largest |x| (relu: of the largest positive value) wherever it sits: in every slot of the
    first vector, of a middle vector and of the last vector; a larger negative value counts without relu only"""
    dt = GEMM_PLANES[mode][0]
    n = 8 * 300                                                      # two blocks
    base = (scaled_values(n, 31).clamp(-3.0, 3.0)).to(dt)
    for vec in (0, 150, 299):
        for slot in range(8):
            x = base.clone()
            x[8 * vec + slot] = 3.5
            x[(8 * vec + slot + 1001) % n] = -7.0
            assert amax_of(mode, x, 1) == f32_bits(3.5), (vec, slot)
            assert amax_of(mode, x, 0) == f32_bits(7.0), (vec, slot)
    x = -base.abs() - 0.25
    assert amax_of(mode, x, 1) == 0                                  # all negative under relu
    assert amax_of(mode, x, 0) == f32_bits(float(x.float().abs().max()))
    assert amax_of(mode, base, 0, initial=f32_bits(100.0)) == f32_bits(100.0)      # a larger value already there stays
    assert amax_of(mode, base, 0, initial=f32_bits(0.5)) == f32_bits(float(base.float().abs().max()))


@pytest.mark.parametrize("mode", ONE_PLANE)
def test_amax_past_the_grid_cap(mode):
    dt = GEMM_PLANES[mode][0]
    n = 4096 * 256 * 8 + 8 * 777
    x = scaled_values(n, 32).clamp(-3.0, 3.0).to(dt)
    want = float(x.float().abs().max())
    assert amax_of(mode, x, 0) == f32_bits(want)
    x[n - 3] = 5.0                                                   # reached only in the second trip of the loop
    x[17] = -6.0
    assert amax_of(mode, x, 1) == f32_bits(5.0)
    assert amax_of(mode, x, 0) == f32_bits(6.0)


def test_amax_refusals():
    x = torch.ones(64, device=DEV, dtype=torch.bfloat16)
    out = torch.zeros(1, device=DEV, dtype=torch.int32)
    for n in (0, 12, -8):
        assert lib().dptx_op_amax(DTYPES["bf16"], ptr(x), n, 0, ptr(out), stream()) == E_INVALID
    assert lib().dptx_op_amax(DTYPES["bf16"], ptr(x), 64, 0, None, stream()) == E_INVALID
    assert lib().dptx_op_amax(9, ptr(x), 64, 0, ptr(out), stream()) == E_INVALID
    torch.cuda.synchronize()
    assert int(out.item()) == 0


# -------------------------------------------------------------------------------------------------------------- nonfinite_scan
NONFINITE = {"bf16": (0x7F80, 0xFF80, 0x7FC0, 0x7F81, 0xFFFF), "fp16": (0x7C00, 0xFC00, 0x7E00, 0x7C01, 0xFFFF)}
LARGEST_FINITE = {"bf16": (0x7F7F, 0xFF7F), "fp16": (0x7BFF, 0xFBFF)}


def scan(mode, bits, initial=0):
    flag = torch.tensor([initial], device=DEV, dtype=torch.int32)
    assert lib().dptx_op_nonfinite_scan(DTYPES[mode], ptr(bits), bits.numel(), ptr(flag), stream()) == 0
    torch.cuda.synchronize()
    return int(flag.item())


def i16(pattern):
    return pattern - 0x10000 if pattern >= 0x8000 else pattern


@pytest.mark.parametrize("mode", ONE_PLANE)
def test_nonfinite_scan(mode):
    """an integer scan of the bit patterns: +Inf, -Inf and three NaN payloads set the flag from the first element, the last
    element and every slot of a middle vector; +-the largest finite number and an all-finite tensor leave it; a flag that
    holds 2 becomes 3 (or stays 2)"""
    dt = GEMM_PLANES[mode][0]
    n = 8 * 300
    clean = scaled_values(n, 41).to(dt).view(torch.int16)
    assert scan(mode, clean) == 0 and scan(mode, clean, 2) == 2
    for pattern in LARGEST_FINITE[mode]:
        x = clean.clone()
        x[::7] = i16(pattern)
        assert scan(mode, x) == 0, hex(pattern)
    for pattern in NONFINITE[mode]:
        for pos in [0, n - 1] + [8 * 150 + s for s in range(8)]:
            x = clean.clone()
            x[pos] = i16(pattern)
            assert scan(mode, x) == 1, (hex(pattern), pos)
        assert scan(mode, x, 2) == 3, hex(pattern)


@pytest.mark.parametrize("mode", ONE_PLANE)
def test_nonfinite_scan_past_the_grid_cap(mode):
    dt = GEMM_PLANES[mode][0]
    n = 2048 * 256 * 8 + 8 * 100
    x = scaled_values(n, 42).to(dt).view(torch.int16)
    assert scan(mode, x) == 0
    x[n - 1] = i16(NONFINITE[mode][3])                               # reached only in the second trip of the loop
    assert scan(mode, x) == 1


def test_nonfinite_scan_refusals():
    x = torch.full((64,), 0x7F80, device=DEV, dtype=torch.int16)
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    for n in (0, 12, -8):
        assert lib().dptx_op_nonfinite_scan(DTYPES["bf16"], ptr(x), n, ptr(flag), stream()) == E_INVALID
    assert lib().dptx_op_nonfinite_scan(DTYPES["bf16"], ptr(x), 64, None, stream()) == E_INVALID
    torch.cuda.synchronize()
    assert int(flag.item()) == 0


# ----------------------------------------------------------------------------------------------------------------- readout_cls
READOUT_CASES = [(3, 64, 768), (2, 192, 1024), (1, 4, 256), (5, 3, 768)]     # (B, N, K); the last: a block with idle waves


@pytest.mark.parametrize("mode,x16", [(m, 0) for m in GEMM_MODES] + [(m, 1) for m in ONE_PLANE])
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("case", READOUT_CASES)
def test_readout_cls_elements(mode, x16, with_bias, case):
    """out[b, n] = sum_k x[b 5K + k] W[n 2K + K + k] + bias[n] within F S of fp64, S = sum |x| |w| + |bias| and F the GEMM's
    fp32 floor: the output is fp32 and w is hi + lo in the plane modes.  Every row and column the launch must not read is NaN."""
    B, N, K = case
    dt, pl = GEMM_PLANES[mode]
    A, Wv, bias, _ = scaled_gemm_operands(B, N, K, seed=K + N)
    nan = float("nan")
    xs = torch.full((B, 5 * K), nan, dtype=torch.float64)
    xs[:, :K] = A
    Wf = torch.full((N, 2 * K), nan, dtype=torch.float64)
    Wf[:, K:] = Wv
    arena = None
    try:
        if pl == 2:
            arena = PlaneArena(Wf.numel() + 4096, DEV, dt)
            Wd = arena.put(Wf)
            w_read = arena.value(Wd).cpu()[:, K:]
        else:
            Wd = Wf.float().to(dt).to(DEV)
            w_read = Wd.double().cpu()[:, K:]
        xd = xs.float().to(dt if x16 else torch.float32).to(DEV)
        bd = bias.float().to(DEV) if with_bias else None
        buf, out = guarded_f32(B * N, 64)
        rc = lib().dptx_op_readout_cls(DTYPES[mode], ptr(xd), 5 * K, ptr(Wd), 2 * K, K, ptr(bd), ptr(out), B, N, K, x16, stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert f32_guards_intact(buf, B * N, 64)
        y, S = gemm_ref64(xd.double().cpu()[:, :K], w_read, bd.cpu() if with_bias else None)
        F = GEMM_F32_FLOOR_FACTOR * GEMM_F32_FLOOR_MEASURED
        assert_elements_inside(out.double().cpu().view(B, N), y, F * S, f"readout_cls {mode} x16={x16} bias={with_bias} {case}")
    finally:
        if arena is not None:
            arena.release()


def test_readout_cls_refusals():
    K, N, B = 256, 4, 1
    x = torch.zeros(B * K, device=DEV)
    W = torch.zeros(N * 2 * K, device=DEV, dtype=torch.bfloat16)
    buf, out = guarded_f32(B * N, 64)
    bf, x3 = DTYPES["bf16"], DTYPES["bf16x3"]
    for args in ((bf, ptr(x), K, ptr(W), 2 * K, K, None, ptr(out), B, N, K - 2, 0), (bf, ptr(x), K, ptr(W), 2 * K, K + 2, None, ptr(out), B, N, K - 4, 0),
                 (bf, ptr(x), K, ptr(W), 2 * K - 2, K - 4, None, ptr(out), B, N, K, 0), (bf, ptr(x), K + 2, ptr(W), 2 * K, K, None, ptr(out), B, N, K, 0),
                 (bf, ptr(x), K, ptr(W), K, K, None, ptr(out), B, N, K, 0), (bf, ptr(x), K, ptr(W), 2 * K, K, None, ptr(out), 0, N, K, 0),
                 (x3, ptr(x), K, ptr(W), 2 * K, K, None, ptr(out), B, N, K, 1), (bf, ptr(x), K, ptr(W), 2 * K, K, None, None, B, N, K, 0)):
        assert lib().dptx_op_readout_cls(*args, stream()) == E_INVALID, args
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


# ------------------------------------------------------------------------------------------------------------------ pos_resize
def run_pos(src, gh, gw):
    C = src.shape[1]
    n = (gh * gw + 1) * C
    buf, dst = guarded_f32(n, C)
    assert lib().dptx_op_pos_resize(ptr(src), ptr(dst), 24, gh, gw, C, stream()) == 0
    torch.cuda.synchronize()
    assert f32_guards_intact(buf, n, C)
    return dst.view(gh * gw + 1, C)


@pytest.mark.parametrize("C", [768, 1024])
def test_pos_resize_identity_is_exact(C):
    src = scaled_pos_embed(C, seed=C).float().to(DEV)
    assert torch.equal(run_pos(src, 24, 24).view(torch.int32), src.view(torch.int32))     # weights 1 and 0 are exact


@pytest.mark.parametrize("C", [768, 1024])
@pytest.mark.parametrize("grid", POS_GRIDS)
def test_pos_resize_elements(C, grid):
    """the cls row copied bit for bit; every grid element within c 2^-24 Sb + e_s L of the fp64 blend at the exact rational
    half-pixel coordinates (gpu_util.pos_resize_ref64 / pos_elem_bound)"""
    src64 = scaled_pos_embed(C, seed=C)
    src = src64.float().to(DEV)
    got = run_pos(src, *grid)
    assert torch.equal(got[0].view(torch.int32), src[0].view(torch.int32))
    y, Sb, L = pos_resize_ref64(src64, 24, *grid)
    assert_elements_inside(got.double().cpu()[1:], y[1:], pos_elem_bound(Sb, L)[1:], f"pos_resize 24 -> {grid} C={C}")


def test_pos_resize_refusals():
    src = torch.zeros(577 * 8, device=DEV)
    buf, dst = guarded_f32(1024, 64)
    for args in ((ptr(src), ptr(dst), 24, 0, 4, 8), (ptr(src), ptr(dst), 24, 4, 4, 0), (ptr(src), ptr(dst), 0, 4, 4, 8),
                 (None, ptr(dst), 24, 4, 4, 8), (ptr(src), ptr(dst), 24, 1 << 15, 1 << 15, 8)):
        assert lib().dptx_op_pos_resize(*args, stream()) == E_INVALID, args
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
