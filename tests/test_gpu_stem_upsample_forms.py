"""The second forms of the stem convolution (csrc/stem.hip stem_conv_kernel_wp: wave-private 16-bit staging, four blocks per
CU) and of the x2 up-sampling (csrc/misc.hip upsample2x_strip_kernel: a strip of output rows per thread, separable blends)
against the kernels they replace (dptx_debug_set_gemm_flags 128: both on their first kernels), bit for bit on the whole
output, with nothing written outside it; against fp32 under the bounds of tests/test_gpu_ops.py; and in the whole forward.
Flag 0 is the forward's dispatch, which takes the strip form only in the (H, C) classes where it measured faster; flag 256
takes it wherever it can run, and dptx_op_upsample2x_strip runs it with either strip height."""
import pytest
import torch
import torch.nn.functional as F

from omnidata_amd.engine import DTYPES, load_library
from tests.gpu_util import OUT_TOL, TDT, ptr, rel_err, stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IO = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}
SENTINEL = 0xFFC1 - 0x10000  # int16 view of 0xFFC1: a NaN in bf16 and in fp16, which neither kernel stores here

# (B, H, W): one block row and one full column tile; Wo = 20, a partial column tile, and the batch stride; Wo = 132, three
# column tiles, the last of 4 columns; the benchmark's width
STEM_CASES = [(1, 8, 128), (3, 16, 40), (2, 24, 264), (1, 32, 384)]
# (B, H, W, C): the degenerate scale; a tiny map; H not a multiple of any strip and odd sizes; two decoder classes
UP_CASES = [(2, 1, 1, 64), (1, 2, 3, 64), (3, 5, 7, 128), (1, 12, 12, 256), (2, 24, 24, 256)]
_cache = {}


class flags:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        assert load_library().dptx_debug_set_gemm_flags(self.value) == 0

    def __exit__(self, *exc):
        load_library().dptx_debug_set_gemm_flags(0)


def guarded(n, guard, dtype):
    """(whole buffer as int16, view of the n payload elements): `guard` sentinel elements in front of and behind the payload,
    the payload pre-filled with the sentinel too"""
    buf = torch.full((guard + n + guard,), SENTINEL, device=DEV, dtype=torch.int16)
    return buf, buf[guard:guard + n].view(TDT[dtype])


def guards_intact(buf, n, guard):
    return bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + n:] == SENTINEL).all())


def stem_operands(dtype, io, case):
    key = ("stem", dtype, io, case)
    if key not in _cache:
        B, H, W = case
        g = torch.Generator(device="cpu").manual_seed(41)
        x = torch.rand(B, 3, H, W, generator=g).to(IO[io][1]).to(DEV)
        w = (torch.randn(64, 3, 7, 7, generator=g) * 147 ** -0.5).to(DEV)
        wp = torch.zeros(64, 176, device=DEV)
        wp[:, :168].view(64, 3, 7, 8)[..., :7] = w                   # k = (c*7 + ky)*8 + kx
        _cache[key] = (x, w.to(TDT[dtype]), wp.to(TDT[dtype]))
    return _cache[key]


def run_stem(dtype, io, case, flag):
    key = ("stem_out", dtype, io, case, flag)
    if key not in _cache:
        B, H, W = case
        x, _, wp = stem_operands(dtype, io, case)
        n, guard = B * (H // 2) * (W // 2) * 64, (W // 2) * 64
        buf, y = guarded(n, guard, dtype)
        with flags(flag):
            rc = load_library().dptx_op_stem_conv_io(DTYPES[dtype], ptr(x), IO[io][0], ptr(wp), ptr(y), B, H, W, stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert guards_intact(buf, n, guard), (case, flag)
        _cache[key] = y.view(B, H // 2, W // 2, 64)
    return _cache[key]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("io", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", STEM_CASES)
def test_stem_new_form_equals_old_bitwise(dtype, io, case):
    new, old = run_stem(dtype, io, case, 0), run_stem(dtype, io, case, 128)
    assert not bool((old.view(torch.int16) == SENTINEL).any())      # the old form wrote every element, so equality means the new did
    assert torch.equal(new.view(torch.int16), old.view(torch.int16))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("io", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", STEM_CASES)
def test_stem_new_form_against_fp32(dtype, io, case):
    """the reference and the bound of tests/test_gpu_ops.py::test_fused_stem_conv: one number per tensor.  Both forms are judged
    element by element, on signed and scaled operands, in tests/test_gpu_stem_elements.py."""
    x, w, _ = stem_operands(dtype, io, case)
    ref = F.conv2d(F.pad(x.float().to(TDT[dtype]).float(), [2, 3, 2, 3]), w.float(), None, 2).permute(0, 2, 3, 1)
    y = run_stem(dtype, io, case, 0)
    assert ref.shape == y.shape
    assert rel_err(y.float(), ref) < OUT_TOL[dtype]


def up_input(dtype, case):
    key = ("up", dtype, case)
    if key not in _cache:
        g = torch.Generator(device="cpu").manual_seed(42)
        _cache[key] = torch.randn(*case, generator=g).to(TDT[dtype]).to(DEV)
    return _cache[key]


def run_up(dtype, case, form):
    """form: ("flag", value) -- dptx_op_upsample2x under that debug flag; ("strip", R) -- the strip form alone"""
    key = ("up_out", dtype, case, form)
    if key not in _cache:
        B, H, W, C = case
        X = up_input(dtype, case)
        n, guard = B * 4 * H * W * C, 2 * W * C
        buf, y = guarded(n, guard, dtype)
        lib = load_library()
        if form[0] == "flag":
            with flags(form[1]):
                rc = lib.dptx_op_upsample2x(DTYPES[dtype], ptr(X), ptr(y), B, H, W, C, stream())
        else:
            rc = lib.dptx_op_upsample2x_strip(DTYPES[dtype], ptr(X), ptr(y), B, H, W, C, form[1], stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert guards_intact(buf, n, guard), (case, form)
        _cache[key] = y.view(B, 2 * H, 2 * W, C)
    return _cache[key]


UP_FORMS = [("flag", 0), ("flag", 256), ("strip", 4), ("strip", 8)]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", UP_CASES)
def test_upsample_new_form_equals_old_bitwise(dtype, case):
    old = run_up(dtype, case, ("flag", 128))
    assert not bool((old.view(torch.int16) == SENTINEL).any())
    for form in UP_FORMS:
        assert torch.equal(run_up(dtype, case, form).view(torch.int16), old.view(torch.int16)), form


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", UP_CASES)
def test_upsample_new_form_against_fp32(dtype, case):
    """the reference and the bound of tests/test_gpu_ops.py::test_upsample2x_align_corners"""
    X = up_input(dtype, case)
    ref = F.interpolate(X.float().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    for form in (("strip", 4), ("strip", 8)):
        assert rel_err(run_up(dtype, case, form).float(), ref) < OUT_TOL[dtype], form


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_whole_forward_old_and_new_forms_equal_bitwise(dtype):
    """B = 3, 384 x 384, one stream and two: first kernels everywhere (128), the forward's dispatch (0), and the strip form
    wherever it can run (256) give the same bits."""
    from omnidata_amd.engine import Engine
    from omnidata_amd.weights import random_state_dict, synthetic_input
    lib = load_library()
    x = synthetic_input(9, 3, "normal").to(DEV)
    sd = random_state_dict(0, 3)
    try:
        for streams in (1, 2):
            eng = Engine(num_channels=3, max_batch=3, dtype=dtype, device_id=0, streams=streams)
            eng.load_state_dict(sd)
            outs = []
            for flag in (128, 0, 256):
                lib.dptx_debug_set_gemm_flags(flag)
                outs.append(eng.forward(x).clone())
            assert torch.isfinite(outs[0]).all(), streams
            assert torch.equal(outs[1], outs[0]), streams
            assert torch.equal(outs[2], outs[0]), streams
            eng.close()
    finally:
        lib.dptx_debug_set_gemm_flags(0)
