"""norm3 folded into a second pass of the streaming 1x1 kernel (csrc/conv1x1.hip, forms C1_STATS and C1_GN; norm.hip
gn_finalize) against the schedule it replaces -- conv3, then the GroupNorm apply pass (dptx_op_conv_groupnorm, on the tiled
kernels with dptx_debug_set_gemm_flags 8 and on the forward's dispatch with 0) -- bit for bit, against fp32, against itself at
another batch size, and in the whole forward (flags 32: never folded, 0: the adopted classes, 64: wherever it can run).
Shapes: the smallest at which the kernel can go wrong -- 96 rows per image (three GroupNorm records; M = 288: a block's four
32-row waves straddle image boundaries and the last block is ragged), M = 32 (one wave of one block has work), and the three
(K, N) classes of the stages' conv3 (one, four and eight W panels)."""
import pytest
import torch
import torch.nn.functional as F

from omnidata_amd.engine import DTYPES, load_library
from tests.gpu_util import OUT_TOL, TDT, ptr, rel_err, stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# B, H, W, Cin, Cout
CASES = [(3, 8, 12, 64, 256), (3, 8, 12, 128, 512), (3, 8, 12, 256, 1024), (1, 4, 8, 64, 256), (1, 4, 8, 256, 1024)]
_cache = {}


def rnd(*shape, dtype, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(TDT[dtype]).to(DEV)


def operands(dtype, case):
    """X, the conv's weight, (gamma, beta); the shortcut R; a second conv's weight and (gamma, beta): the downsample branch"""
    B, H, W, Cin, Cout = case
    key = ("ops", dtype, case)
    if key not in _cache:
        g = torch.Generator(device="cpu").manual_seed(43)
        vec = lambda: torch.randn(Cout, generator=g).to(DEV)
        _cache[key] = (rnd(B, H, W, Cin, dtype=dtype, seed=40), rnd(Cout, 1, 1, Cin, dtype=dtype, scale=Cin ** -0.5, seed=41), vec(), vec(),
                       rnd(B, H, W, Cout, dtype=dtype, seed=42), rnd(Cout, 1, 1, Cin, dtype=dtype, scale=Cin ** -0.5, seed=44), vec(), vec())
    return _cache[key]


def run_unfused(dtype, case, flags, res, relu, image=None, second=False):
    """(raw map, Y, records) of dptx_op_conv_groupnorm -- conv, then the apply pass; second: the downsample branch's conv"""
    key = ("unfused", dtype, case, flags, res, relu, image, second)
    if key in _cache:
        return _cache[key]
    lib = load_library()
    B, H, W, Cin, Cout = case
    X, Wt, g, b, R, W2, g2, b2 = operands(dtype, case)
    if second:
        Wt, g, b = W2, g2, b2
    if image is not None:
        X, R, B = X[image:image + 1].contiguous(), R[image:image + 1].contiguous(), 1
    Yraw = torch.empty(B, H, W, Cout, device=DEV, dtype=TDT[dtype])
    Y = torch.empty_like(Yraw)
    rec = torch.full((B, H * W // 32, 32, 2), float("nan"), device=DEV)
    try:
        assert lib.dptx_debug_set_gemm_flags(flags) == 0
        rc = lib.dptx_op_conv_groupnorm(DTYPES[dtype], ptr(X), ptr(Wt), ptr(Yraw), ptr(g), ptr(b), ptr(R) if res else None, ptr(Y),
                                        B, H, W, Cin, Cout, 1, 1, 0, 0, H, W, relu, 1e-5, ptr(rec), stream())
    finally:
        lib.dptx_debug_set_gemm_flags(0)
    assert rc == 0
    torch.cuda.synchronize()
    _cache[key] = (Yraw, Y, rec)
    return _cache[key]


def run_fused(dtype, case, res, relu, image=None, passes=7, sentinel=None):
    """(Y, records, tables) of dptx_op_conv_groupnorm_fused; res: 0 none, 1 R, 2 R behind its own GroupNorm (the records of
    the second conv, as dptx_op_conv_groupnorm leaves them)"""
    key = ("fused", dtype, case, res, relu, image, passes, sentinel)
    if key in _cache:
        return _cache[key]
    lib = load_library()
    B, H, W, Cin, Cout = case
    X, Wt, g, b, R, W2, g2, b2 = operands(dtype, case)
    r_rec = None
    if res == 2:
        R, _, r_rec = run_unfused(dtype, case, 8, 0, 0, image, second=True)   # R = the second conv's raw map
    elif image is not None:
        R = R[image:image + 1].contiguous()
    if image is not None:
        X, B = X[image:image + 1].contiguous(), 1
    Y = torch.empty(B, H, W, Cout, device=DEV, dtype=TDT[dtype])
    if sentinel is not None:
        Y.fill_(sentinel)
    rec = torch.full((B, H * W // 32, 32, 2), float("nan"), device=DEV)
    tab = torch.full((B, 4, Cout), float("nan"), device=DEV)
    rc = lib.dptx_op_conv_groupnorm_fused(DTYPES[dtype], ptr(X), ptr(Wt), ptr(g), ptr(b), ptr(R) if res else None,
                                          ptr(g2) if res == 2 else None, ptr(b2) if res == 2 else None, ptr(r_rec), ptr(Y), B, H, W,
                                          Cin, Cout, relu, 1e-5, ptr(rec), ptr(tab), passes, stream())
    assert rc == 0
    torch.cuda.synchronize()
    _cache[key] = (Y, rec, tab)
    return _cache[key]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES)
def test_fused_equals_unfused_bitwise(dtype, case):
    """no shortcut, a plain shortcut (the later blocks of a stage), ReLU off and on; against the tiled kernels (flag 8) and
    the forward's dispatch (flag 0)"""
    for res, relu in ((0, 0), (0, 1), (1, 1), (1, 0)):
        new = run_fused(dtype, case, res, relu)
        for flags in (8, 0):
            old = run_unfused(dtype, case, flags, res, relu)
            assert torch.equal(new[0], old[1]), (res, relu, flags)
            assert torch.equal(new[1], old[2]), (res, relu, flags)       # the records
        assert not torch.isnan(new[2][:, :2]).any()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES)
def test_fused_downsample_form_equals_the_apply_pass_bitwise(dtype, case):
    """the shortcut behind a GroupNorm of its own (the first block of a stage): the fold against the schedule it replaces
    there -- conv3 and the downsample convolution on the tiled kernels, then dptx_op_groupnorm_records, the apply pass the
    forward launches on their raw maps and records"""
    lib = load_library()
    B, H, W, Cin, Cout = case
    _, _, g, b, _, _, g2, b2 = operands(dtype, case)
    raw, _, rec = run_unfused(dtype, case, 8, 0, 0)
    R, _, r_rec = run_unfused(dtype, case, 8, 0, 0, second=True)
    for relu in (0, 1):
        Y = torch.full_like(raw, float("nan"))
        rc = lib.dptx_op_groupnorm_records(DTYPES[dtype], ptr(raw), ptr(g), ptr(b), ptr(rec), ptr(R), ptr(g2), ptr(b2), ptr(r_rec), ptr(Y),
                                           B, H * W, Cout, relu, 1e-5, stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(Y, run_fused(dtype, case, 2, relu)[0]), relu


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES)
def test_stats_pass_writes_the_records_and_nothing_else(dtype, case):
    Y, rec, _ = run_fused(dtype, case, 0, 0, passes=1, sentinel=3.0)
    old = run_unfused(dtype, case, 16, 0, 0)                             # the storing form of the same kernel
    assert torch.equal(rec, old[2]) and torch.equal(rec, run_unfused(dtype, case, 8, 0, 0)[2])
    assert not torch.isnan(rec).any()
    assert bool((Y == 3.0).all())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES)
def test_finalize_gives_the_affines_of_the_records(dtype, case):
    """tables = (rstd gamma, beta - mean rstd gamma) of the fp64 statistics of the records; rows 2 / 3 only with r_records"""
    B, H, W, Cin, Cout = case
    _, _, g, b, _, _, g2, b2 = operands(dtype, case)
    for res in (1, 2):
        _, rec, tab = run_fused(dtype, case, res, 1)
        recs = [(rec, g, b)] + ([(run_unfused(dtype, case, 8, 0, 0, second=True)[2], g2, b2)] if res == 2 else [])
        for t, (r, gm, bt) in enumerate(recs):
            n = H * W * (Cout // 32)
            mean = r[..., 0].double().sum(1) / n
            var = (r[..., 1].double().sum(1) / n - mean * mean).clamp_min(0)
            a = (torch.rsqrt(var + 1e-5).repeat_interleave(Cout // 32, 1) * gm.double())
            d = bt.double() - mean.repeat_interleave(Cout // 32, 1) * a
            assert rel_err(tab[:, 2 * t], a) < 1e-6 and rel_err(tab[:, 2 * t + 1], d) < 1e-6
        assert bool(torch.isnan(tab[:, 2:]).all()) == (res == 1)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES)
def test_fused_against_fp32(dtype, case):
    """The bound and the form of test_gpu_conv1x1_stream.py::test_stream_conv_groupnorm_against_fp32: group_norm's fp32
    statistics of the fp32 convolution applied to the rounded map.  Also with the shortcut behind a GroupNorm of its own (the
    first block of a stage); its bitwise check against the apply pass is test_fused_downsample_form_equals_the_apply_pass_bitwise."""
    B, H, W, Cin, Cout = case
    X, Wt, g, b, R, W2, g2, b2 = operands(dtype, case)

    def gn32(w, gm, bt):
        raw = F.conv2d(X.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        xr = raw.permute(0, 3, 1, 2).reshape(B, 32, -1)
        mean, var = xr.mean(-1), xr.var(-1, unbiased=False)
        a = gm.view(1, -1) * torch.rsqrt(var + 1e-5).repeat_interleave(Cout // 32, 1)
        d = bt.view(1, -1) - mean.repeat_interleave(Cout // 32, 1) * a
        return raw.to(TDT[dtype]).float() * a.view(B, 1, 1, Cout) + d.view(B, 1, 1, Cout)

    main = gn32(Wt, g, b)
    assert rel_err(run_fused(dtype, case, 0, 1)[0].float(), F.relu(main)) < OUT_TOL[dtype]
    assert rel_err(run_fused(dtype, case, 1, 1)[0].float(), F.relu(main + R.float())) < OUT_TOL[dtype]
    assert rel_err(run_fused(dtype, case, 2, 1)[0].float(), F.relu(main + gn32(W2, g2, b2))) < OUT_TOL[dtype]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", [c for c in CASES if c[0] == 3])
def test_fused_batch_invariance_bitwise(dtype, case):
    """image 1 of the batch of three == the same image run alone: output, records, tables; all three shortcut forms"""
    for res in (0, 1, 2):
        full, one = run_fused(dtype, case, res, 1), run_fused(dtype, case, res, 1, image=1)
        for f, o in zip(full, one):
            assert torch.equal(f[1].view(torch.int32) if f.dtype == torch.float32 else f[1],
                               o[0].view(torch.int32) if o.dtype == torch.float32 else o[0]), res   # (NaN rows of the tables: as bits)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_whole_forward_folded_equals_unfolded_bitwise(dtype):
    """Whole forward at B = 3, 384 x 384, on one stream and on two: never folded (flag 32, the schedule conv3 -> apply pass),
    the adopted classes (0) and every eligible conv3 (64: all 16 bottlenecks, the first block of each stage with the
    downsample branch's GroupNorm in the epilogue) give the same bits."""
    from omnidata_amd.engine import Engine
    from omnidata_amd.weights import random_state_dict, synthetic_input
    lib = load_library()
    x = synthetic_input(9, 3, "normal").to(DEV)
    sd = random_state_dict(0, 3)
    try:
        for streams in (1, 2):
            eng = Engine(num_channels=3, max_batch=3, dtype=dtype, device_id=0, streams=streams)
            eng.load_state_dict(sd)
            outs, launches = [], []
            for flags in (32, 0, 64):
                lib.dptx_debug_set_gemm_flags(flags)
                outs.append(eng.forward(x).clone())
                launches.append(eng.info()[0])
            assert torch.isfinite(outs[0]).all(), streams
            assert torch.equal(outs[1], outs[0]), streams
            assert torch.equal(outs[2], outs[0]), streams
            assert launches[2] == launches[0] + 16 * streams, (streams, launches)   # 2 launches -> 3 in all 16 bottlenecks
            eng.close()
    finally:
        lib.dptx_debug_set_gemm_flags(0)
