"""The kernels that interpolate -- the fused head tail (csrc/head.hip), the 1x1 projection of the unfused tail and the x2
up-sampling in all its forms (csrc/misc.hip) -- judged element by element against fp64.

Operands carry a scale of their own in every pixel and channel (tests/gpu_util.scaled_head_operands), the w4 rows are scaled
8, 1, 1/8, so a small pixel, channel or output channel is judged by its own size.  Every output element must lie within
up_elem_bound / head_elem_bound of the fp64 value of the expression on the values the kernel actually reads.  The window claim
of head.hip -- the up-sampled window holds the bits upsample2x_kernel stores -- is tested directly with one-hot weights
(test_head_window_probe).  What the bounds are worth -- which mistakes they reject -- is shown on a CPU in
tests/test_head_bound_host.py; profiles/head_elements.md has the figures.  Outputs start as NaN between sentinel guards, inputs
are followed by NaN: an element that is not written, a write outside the payload or a read behind the input fails.
pytest -m gpu."""
import functools

import pytest
import torch
import torch.nn.functional as F

from omnidata_amd.engine import DTYPES, load_library
from tests.gpu_util import (GEMM_F32_FLOOR_FACTOR, GEMM_F32_FLOOR_MEASURED, GEMM_MODES, GEMM_PLANES, HEAD_HOST_SHAPES, UP_VARIANTS,
                            PlaneArena, assert_elements_inside, head_elem_bound, head_out_ref64, head_tail_ref64, ptr,
                            scaled_head_operands, stream, upsample_variants_inside)
from tests.test_gpu_stem_upsample_forms import UP_CASES, flags

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENTINEL = 0xFFC1 - 0x10000  # int16 view of 0xFFC1: a NaN in bf16 and in fp16 that no kernel stores here
IO = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}
HEAD_MODES = ("bf16", "fp16", "fp16x3")


class Arena(PlaneArena):
    """PlaneArena in every mode (the one-plane modes read and write the hi plane) with guarded tensors."""

    def __init__(self, mode, elems):
        self.dt, self.pl = GEMM_PLANES[mode]
        super().__init__(elems + 8192, dtype=self.dt)
        self.outs = []

    def val(self, t):
        """fp64 value of what a kernel reads from / wrote to t"""
        return self.value(t) if self.pl == 2 else t.double()

    def put_guarded(self, t, guard):
        """put(t), followed by `guard` NaN elements in both planes: a read behind the tensor shows"""
        x = self.put(t)
        g = self.empty(guard)
        g.view(torch.int16).fill_(SENTINEL)
        self.lo(g).view(torch.int16).fill_(SENTINEL)
        return x

    def out(self, shape, guard):
        """a tensor of `shape` pre-filled with the sentinel NaN, `guard` sentinel elements in front of and behind it, in both planes"""
        n = 1
        for s in shape:
            n *= s
        full = self.empty(guard + n + guard)
        full.view(torch.int16).fill_(SENTINEL)
        self.lo(full).view(torch.int16).fill_(SENTINEL)
        self.outs.append((full, n, guard))
        return full[guard:guard + n].view(*shape)

    def guards_intact(self):
        """every guard of every out() tensor still holds the sentinel -- and, in the one-plane modes, the whole lo plane of it"""
        for full, n, guard in self.outs:
            for plane in (full, self.lo(full)):
                p = plane.view(torch.int16)
                if not (bool((p[:guard] == SENTINEL).all()) and bool((p[guard + n:] == SENTINEL).all())):
                    return False
            if self.pl == 1 and not bool((self.lo(full).view(torch.int16) == SENTINEL).all()):
                return False
        return True


def guarded_buffer(shape, guard, io="fp32"):
    """(whole buffer, payload view of `shape`) outside the arena: fp32 NaN, or the 16-bit sentinel for a 16-bit io type"""
    n = 1
    for s in shape:
        n *= s
    if io == "fp32":
        buf = torch.full((guard + n + guard,), NAN, device=DEV)
        return buf, buf[guard:guard + n].view(*shape)
    buf = torch.full((guard + n + guard,), SENTINEL, device=DEV, dtype=torch.int16)
    return buf, buf[guard:guard + n].view(IO[io][1]).view(*shape)


def buffer_guards_intact(buf, payload, guard):
    n = payload.numel()
    if buf.dtype == torch.float32:
        return bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all())
    return bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + n:] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def head_operands(B, Hs, Ws, C):
    return scaled_head_operands(B, Hs, Ws, C)


def upsample(lib, ar, mode, X, case, form=("flag", 128)):
    """one launch of the x2 up-sampling of X (arena tensor) into a guarded arena tensor [B, 2H, 2W, C].
    form: ("flag", value) -- dptx_op_upsample2x under that debug flag; ("strip", R) -- the strip form alone"""
    B, H, W, C = case
    Y = ar.out((B, 2 * H, 2 * W, C), 2 * W * C)
    if form[0] == "flag":
        with flags(form[1]):
            rc = lib.dptx_op_upsample2x(DTYPES[mode], ptr(X), ptr(Y), B, H, W, C, stream())
    else:
        rc = lib.dptx_op_upsample2x_strip(DTYPES[mode], ptr(X), ptr(Y), B, H, W, C, form[1], stream())
    assert rc == 0, (mode, case, form, rc)
    return Y


# ------------------------------------------------------------------------------------------------------------ x2 up-sampling
# UP_CASES of tests/test_gpu_stem_upsample_forms.py (the degenerate scale, a tiny map, odd sizes, two decoder classes) plus:
# the smallest head source; the largest src coordinate of the forward (96 x 96); odd sizes with C = 8, one vector per pixel
# (cshift = 0) and H = 9 rows, where a strip of 8 is cut short twice (18 = 8 + 8 + 2)
UP_ELEM_CASES = list(UP_CASES) + [(1, 4, 16, 128), (1, 96, 96, 128), (2, 9, 11, 8)]
UP_FORMS = {1: (("flag", 128), ("flag", 256), ("strip", 4), ("strip", 8)), 2: (("flag", 0),)}
_up_results = {}


def up_results(mode, case):
    """{form: (worst |err| / bound per variant, set of variants that hold every element)} of one case, all forms of the mode"""
    if (mode, case) not in _up_results:
        lib = load_library()
        B, H, W, C = case
        pl = GEMM_PLANES[mode][1]
        n = B * H * W * C
        ar = Arena(mode, n + 2 * W * C + len(UP_FORMS[pl]) * (4 * n + 4 * W * C + 256) + 4096)
        try:
            X = ar.put_guarded(scaled_head_operands(B, H, W, 1, 0, C)[0], 2 * W * C)
            Xv = ar.val(X)
            res = {}
            for form in UP_FORMS[pl]:
                Y = upsample(lib, ar, mode, X, case, form)
                torch.cuda.synchronize()
                assert ar.guards_intact(), (mode, case, form)
                res[form] = upsample_variants_inside(ar.val(Y), Xv, mode)
            _up_results[(mode, case)] = res
        finally:
            ar.release()
    return _up_results[(mode, case)]


@pytest.mark.parametrize("mode", GEMM_MODES)
@pytest.mark.parametrize("case", UP_ELEM_CASES)
def test_upsample_elements(mode, case):
    """every element of every form inside up_elem_bound of upsample_ref64 for ONE variant of l1 throughout the launch"""
    for form, (worst, inside) in up_results(mode, case).items():
        print(f"\n[elements] upsample {mode} {case} {form[0]} {form[1]}: worst |err| / bound "
              + ", ".join(f"{worst[v]:.3f} ({UP_VARIANTS[v]})" for v in range(4)))
        assert inside, (mode, case, form, worst)


@pytest.mark.parametrize("mode", GEMM_MODES)
def test_upsample_variant_is_one_per_mode(mode):
    """one variant of l1 holds every element of every case and every form of the mode: the forms use ONE arithmetic"""
    common = set(range(4))
    for case in UP_ELEM_CASES:
        for form, (worst, inside) in up_results(mode, case).items():
            common &= inside
    print(f"\n[elements] upsample {mode}: variants that hold everywhere {[UP_VARIANTS[v] for v in sorted(common)]}")
    assert common, mode


# ----------------------------------------------------------------------------------------------------------------- head tail
# The persistent runs: more tiles than CUs and not a multiple of them, so blocks walk runs of two or more tiles and the last
# blocks get nothing.  "persistent" is (5, 36, 96, 3, 1), 54 tiles per image, 270 on 256 CUs: runs of two, which start at even
# tiles and so never straddle two images.  "persistent-crossing" is (6, 36, 80, 3, 1), 45 tiles per image, 270 again: the run
# (44, 45) crosses from image 0 into image 1, and every second image boundary likewise.  B grows on a device with more CUs.
PERSISTENT = {"persistent": (5, 36, 96, 3, 1), "persistent-crossing": (6, 36, 80, 3, 1)}


def head_shapes():
    return list(HEAD_HOST_SHAPES) + list(PERSISTENT)


def resolve(shape):
    if shape not in PERSISTENT:
        return shape
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B, Hs, Ws, C, relu = PERSISTENT[shape]
    tpi = (2 * Hs // 8) * (2 * Ws // 32)
    crossing = shape == "persistent-crossing"
    while tpi * B <= cus or (tpi * B) % cus == 0 or (crossing and tpi % -(-tpi * B // cus) == 0):
        B += 1
    ntiles = tpi * B
    assert ntiles > cus and ntiles % cus != 0, (ntiles, cus)
    assert not crossing or tpi % -(-ntiles // cus) != 0, "no run crosses an image boundary"
    return (B, Hs, Ws, C, relu)


def head_arena(mode, shape, extra=0):
    B, Hs, Ws, C, _ = shape
    n = B * Hs * Ws * 128
    return Arena(mode, 2 * n + 4 * Ws * 128 + 4 * n + 8 * Ws * 128 + 2 * 32 * 9 * 128 + extra + 8192)


def head_setup(lib, ar, mode, shape):
    """arena operands of one head case and the up-sampled map U (first kernel, flag 128) of H0"""
    B, Hs, Ws, C, _ = shape
    H64, W64, b2, w4, b4 = head_operands(B, Hs, Ws, C)
    H0 = ar.put_guarded(H64, 2 * Ws * 128)
    W2 = ar.put(W64)
    U = upsample(lib, ar, mode, H0, (B, Hs, Ws, 128))
    return H0, W2, b2.float().to(DEV), w4.float().to(DEV), b4.float().to(DEV), U


def run_head(lib, mode, H0, W2, b2, w4, b4, shape, relu, io="fp32"):
    B, Hs, Ws, C, _ = shape
    buf, y = guarded_buffer((B, C, 2 * Hs, 2 * Ws), 2 * Ws, io)
    if io == "fp32":
        rc = lib.dptx_op_head_tail(DTYPES[mode], ptr(H0), ptr(W2), ptr(b2), ptr(w4), ptr(b4), ptr(y), B, Hs, Ws, C, relu, stream())
    else:
        rc = lib.dptx_op_head_tail_io(DTYPES[mode], ptr(H0), ptr(W2), ptr(b2), ptr(w4), ptr(b4), ptr(y), IO[io][0], B, Hs, Ws, C,
                                      relu, stream())
    assert rc == 0, (mode, shape, io, rc)
    torch.cuda.synchronize()
    assert buffer_guards_intact(buf, y, 2 * Ws), (mode, shape, io)
    return y


# channels of the window probe: 0, 7, 8, 37, 64, 100, 127 and one in every other 8-channel chunk -- all sixteen chunks, all four
# channel quarters of head_tail_x3_kernel
PROBE_CHANNELS = (0, 7, 8, 19, 26, 37, 45, 50, 59, 64, 77, 85, 92, 100, 108, 118, 127)


@pytest.mark.parametrize("mode", HEAD_MODES)
@pytest.mark.parametrize("shape", HEAD_HOST_SHAPES)
def test_head_window_probe(mode, shape):
    """head.hip's claim, directly: the window holds the bits upsample2x_kernel stores.  W2 is one-hot -- output channel n reads
    channel c at ONE tap (ky, kx), its lo plane zero --, b2 = 0, w4 one-hot, b4 = 0, no final ReLU: every MFMA sum is exact (hi + lo
    is an fp32 number), so y(H0) - y(-H0) -- the hidden ReLU keeps one of the two -- must EQUAL the value dptx_op_upsample2x
    (flag 128) stored at [b, oy + ky - 1, ox + kx - 1, c], and 0 outside the image.  All nine taps x PROBE_CHANNELS, the hidden
    channel n walking over all 32."""
    lib = load_library()
    assert {c // 8 for c in PROBE_CHANNELS} == set(range(16))
    B, Hs, Ws, C, _ = shape
    Ho, Wo = 2 * Hs, 2 * Ws
    ar = head_arena(mode, shape)
    try:
        H64 = head_operands(B, Hs, Ws, C)[0]
        Hp, Hn = ar.put_guarded(H64, 2 * Ws * 128), ar.put_guarded(-H64, 2 * Ws * 128)
        W2 = ar.put(torch.zeros(32, 3, 3, 128))
        U = upsample(lib, ar, mode, Hp, (B, Hs, Ws, 128))
        torch.cuda.synchronize()
        Uv = ar.val(U)
        U32 = Uv.float()
        assert torch.equal(U32.double(), Uv)
        Up = F.pad(U32, [0, 0, 1, 1, 1, 1])
        zeros32, zerosC = torch.zeros(32, device=DEV), torch.zeros(C, device=DEV)
        w4 = torch.zeros(C, 32, device=DEV)
        bufs = [guarded_buffer((B, C, Ho, Wo), Wo) for _ in range(2)]
        probes = [(tap, c) for c in PROBE_CHANNELS for tap in range(9)]
        verdicts, names = [], []
        for j0 in range(0, len(probes), C):
            group = probes[j0:j0 + C]
            W2.zero_()
            w4.zero_()
            for i, (tap, c) in enumerate(group):
                n = (5 * (j0 + i)) % 32
                W2[n, tap // 3, tap % 3, c] = 1.0
                w4[i, n] = 1.0
            for (buf, y), H in zip(bufs, (Hp, Hn)):
                y.fill_(NAN)
                rc = lib.dptx_op_head_tail(DTYPES[mode], ptr(H), ptr(W2), ptr(zeros32), ptr(w4), ptr(zerosC), ptr(y), B, Hs, Ws, C, 0, stream())
                assert rc == 0, rc
            ypos, yneg = bufs[0][1], bufs[1][1]
            for i, (tap, c) in enumerate(group):
                ky, kx = tap // 3, tap % 3
                want = Up[:, ky:ky + Ho, kx:kx + Wo, c]
                ok = ((ypos[:, i] - yneg[:, i]) == want).all() & (torch.minimum(ypos[:, i], yneg[:, i]) == 0).all()
                verdicts.append(ok)
                names.append((ky, kx, c, (5 * (j0 + i)) % 32))
            for i in range(len(group), C):       # a one-hot row that is not used: the channel is exactly 0
                verdicts.append((ypos[:, i] == 0).all() & (yneg[:, i] == 0).all())
                names.append(("unused output channel", i))
        torch.cuda.synchronize()
        verdicts = torch.stack(verdicts).cpu().tolist()
        bad = [n for n, ok in zip(names, verdicts) if not ok]
        print(f"\n[window] {mode} {shape}: {len(verdicts) - len(bad)} of {len(verdicts)} probes (ky, kx, channel, n) equal")
        assert not bad, f"{mode} {shape}: the window differs from upsample2x_kernel's output at (ky, kx, channel, n) {bad[:10]}"
        assert all(buffer_guards_intact(buf, y, Wo) for buf, y in bufs) and ar.guards_intact()
    finally:
        ar.release()


@pytest.mark.parametrize("mode", HEAD_MODES)
@pytest.mark.parametrize("shape", head_shapes(), ids=str)
def test_head_tail_elements(mode, shape):
    """dptx_op_head_tail with the scaled operands: every element inside head_elem_bound of head_tail_ref64 on the map U that
    dptx_op_upsample2x (flag 128; judged in test_upsample_elements) gives for the same H0"""
    lib = load_library()
    shape = resolve(shape)
    B, Hs, Ws, C, relu = shape
    ar = head_arena(mode, shape)
    try:
        H0, W2, b2, w4, b4, U = head_setup(lib, ar, mode, shape)
        y = run_head(lib, mode, H0, W2, b2, w4, b4, shape, relu)
        assert ar.guards_intact()
        ref, Sw, Hw, _ = head_tail_ref64(ar.val(U), ar.val(W2), b2, w4, b4, relu)
        bound = head_elem_bound(mode, ref, Sw, Hw)
        print(f"\n[elements] median bound / |y| over y != 0: {float((bound / ref.abs())[ref != 0].median()):.2e}")
        assert_elements_inside(y, ref, bound, f"head tail {mode} {shape}")
    finally:
        ar.release()


def test_head_tail_refuses_bf16x3():
    """bf16x3 keeps the three-launch tail: the fused entry returns an error and writes nothing"""
    lib = load_library()
    shape = HEAD_HOST_SHAPES[1]
    B, Hs, Ws, C, relu = shape
    ar = head_arena("bf16x3", shape)
    try:
        H64, W64, b2, w4, b4 = head_operands(B, Hs, Ws, C)
        H0, W2 = ar.put(H64), ar.put(W64)
        buf, y = guarded_buffer((B, C, 2 * Hs, 2 * Ws), 2 * Ws)
        rc = lib.dptx_op_head_tail(DTYPES["bf16x3"], ptr(H0), ptr(W2), ptr(b2.float().to(DEV)), ptr(w4.float().to(DEV)),
                                   ptr(b4.float().to(DEV)), ptr(y), B, Hs, Ws, C, relu, stream())
        torch.cuda.synchronize()
        assert rc != 0
        assert bool(torch.isnan(buf).all())
    finally:
        ar.release()


@pytest.mark.parametrize("mode", HEAD_MODES)
@pytest.mark.parametrize("io", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [HEAD_HOST_SHAPES[1], HEAD_HOST_SHAPES[3]])
def test_head_tail_io_16bit(mode, io, shape):
    """dptx_op_head_tail_io with a 16-bit result: the bits of the fp32 result rounded to that type by torch; an unknown io is
    refused"""
    lib = load_library()
    B, Hs, Ws, C, relu = shape
    ar = head_arena(mode, shape)
    try:
        H0, W2, b2, w4, b4, _ = head_setup(lib, ar, mode, shape)
        y32 = run_head(lib, mode, H0, W2, b2, w4, b4, shape, relu)
        y16 = run_head(lib, mode, H0, W2, b2, w4, b4, shape, relu, io)
        assert bool(torch.isfinite(y32).all())
        want = y32.to(IO[io][1])
        assert bool(torch.isfinite(want.float()).all())
        diff = want.view(torch.int16) != y16.view(torch.int16)
        print(f"\n[io] head tail {mode} {shape} -> {io}: {int(diff.sum())} of {diff.numel()} elements differ from torch's rounding")
        assert not bool(diff.any()), torch.nonzero(diff)[:5].tolist()
        assert lib.dptx_op_head_tail_io(DTYPES[mode], ptr(H0), ptr(W2), ptr(b2), ptr(w4), ptr(b4), ptr(y32), 3, B, Hs, Ws, C, relu,
                                        stream()) == -1
    finally:
        ar.release()


# ----------------------------------------------------------------------------------------- the 1x1 projection of the unfused tail
# (B, HW): one pixel per image; less than a block; the grid-stride tail; more pixels than the 16384-block grid covers in one pass
HEAD_OUT_SIZES = [(2, 1), (3, 255), (1, 4096 + 3), (1, 16384 * 256 + 8)]


def head_out_input(B, HW):
    """X [B, HW, 32] fp32 on the device, |N(0, 1)| (X is behind a ReLU) with the row scale 2^((7 p mod 13) - 6) of the flat pixel
    index and the channel scale 2^((5 k mod 7) - 3); generated on the device (134 M values at the largest size)"""
    g = torch.Generator(device=DEV).manual_seed(5000 + HW)
    x = torch.randn(B * HW, 32, generator=g, device=DEV).abs_()
    x *= torch.exp2(((7 * torch.arange(B * HW, device=DEV)) % 13 - 6).float())[:, None]
    x *= torch.exp2(((5 * torch.arange(32, device=DEV)) % 7 - 3).float())[None, :]
    return x.view(B, HW, 32)


@pytest.mark.parametrize("mode", GEMM_MODES)
@pytest.mark.parametrize("B,HW", HEAD_OUT_SIZES)
def test_head_out_elements(mode, B, HW):
    """dptx_op_head_out, Cout in {1, 3, 4} x both relu values, fp32 result: every element within F (sum |w| |x| + |b|) of fp64
    (F = the GEMM floor with its margin; x = hi + lo is formed exactly).  On the small sizes also the 16-bit results: the bits of
    the fp32 result rounded by torch.  Cout outside 1..4 and an unknown io are refused."""
    lib = load_library()
    Fl = GEMM_F32_FLOOR_FACTOR * GEMM_F32_FLOOR_MEASURED
    ar = Arena(mode, B * HW * 32 + 4096)
    try:
        X = ar.put_guarded(head_out_input(B, HW), 256)
        Xlo = ar.lo(X) if ar.pl == 2 else None
        g = torch.Generator().manual_seed(77)
        for Cout in (1, 3, 4):
            w = (torch.randn(Cout, 32, generator=g) * torch.tensor([8.0, 1.0, 0.125, 1.0])[:Cout, None] * 32 ** -0.5).to(DEV)
            b = (torch.randn(Cout, generator=g) * torch.tensor([8.0, 1.0, 0.125, 1.0])[:Cout]).to(DEV)
            for relu in (0, 1):
                buf, y = guarded_buffer((B, Cout, HW), 64)
                rc = lib.dptx_op_head_out(DTYPES[mode], ptr(X), ptr(w), ptr(b), ptr(y), 0, B, HW, Cout, relu, stream())
                assert rc == 0, rc
                torch.cuda.synchronize()
                assert buffer_guards_intact(buf, y, 64)
                ref, S = head_out_ref64(X, Xlo, w, b, relu)
                assert_elements_inside(y, ref, Fl * S, f"head out {mode} B={B} HW={HW} Cout={Cout} relu={relu}")
                del ref, S
                if HW > 5000:
                    continue
                for io in ("bf16", "fp16"):
                    buf16, y16 = guarded_buffer((B, Cout, HW), 64, io)
                    assert lib.dptx_op_head_out(DTYPES[mode], ptr(X), ptr(w), ptr(b), ptr(y16), IO[io][0], B, HW, Cout, relu, stream()) == 0
                    torch.cuda.synchronize()
                    assert buffer_guards_intact(buf16, y16, 64)
                    diff = y.to(IO[io][1]).view(torch.int16) != y16.view(torch.int16)
                    assert not bool(diff.any()), (mode, HW, Cout, relu, io, int(diff.sum()), torch.nonzero(diff)[:5].tolist())
        for Cout, io in ((0, 0), (5, 0), (3, 3), (3, -1)):
            assert lib.dptx_op_head_out(DTYPES[mode], ptr(X), ptr(w), ptr(b), ptr(y), io, B, HW, Cout, 0, stream()) == -1
    finally:
        ar.release()


# --------------------------------------------------------------------------------------------------------- the unfused chain
@pytest.mark.parametrize("mode", GEMM_MODES)
@pytest.mark.parametrize("shape", head_shapes(), ids=str)
def test_unfused_chain_elements(mode, shape):
    """dptx_op_upsample2x -> dptx_op_conv (N = 32, ReLU) -> dptx_op_head_out, what bf16x3 and every size the fused form refuses
    run, against head_tail_ref64 on its own up-sampled map; h is stored in the plane(s), which the bound's h_planes terms cover.
    Where the fused form exists it runs on the same operands: each result inside its OWN bound, no bar between the two."""
    lib = load_library()
    shape = resolve(shape)
    B, Hs, Ws, C, relu = shape
    Ho, Wo = 2 * Hs, 2 * Ws
    ar = head_arena(mode, shape, extra=B * Ho * Wo * 32 + 4 * Wo * 32)
    try:
        H64, W64, b2, w4, b4 = head_operands(B, Hs, Ws, C)
        H0 = ar.put_guarded(H64, 2 * Ws * 128)
        W2 = ar.put(W64)
        b2, w4, b4 = b2.float().to(DEV), w4.float().to(DEV), b4.float().to(DEV)
        U = upsample(lib, ar, mode, H0, (B, Hs, Ws, 128), ("flag", 0))
        h = ar.out((B, Ho, Wo, 32), 2 * Wo * 32)
        rc = lib.dptx_op_conv(DTYPES[mode], ptr(U), ptr(W2), ptr(b2), None, ptr(h), B, Ho, Wo, 128, 32, 3, 1, 1, 1, Ho, Wo, 0, 1, stream())
        assert rc == 0, rc
        buf, y = guarded_buffer((B, C, Ho, Wo), Wo)
        rc = lib.dptx_op_head_out(DTYPES[mode], ptr(h), ptr(w4), ptr(b4), ptr(y), 0, B, Ho * Wo, C, relu, stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert ar.guards_intact() and buffer_guards_intact(buf, y, Wo)
        ref, Sw, Hw, Hh = head_tail_ref64(ar.val(U), ar.val(W2), b2, w4, b4, relu)
        assert_elements_inside(y, ref, head_elem_bound(mode, ref, Sw, Hw, h_planes=ar.pl, Hh=Hh), f"unfused chain {mode} {shape}")
        if mode in HEAD_MODES:
            yf = run_head(lib, mode, H0, W2, b2, w4, b4, shape, relu)
            assert_elements_inside(yf, ref, head_elem_bound(mode, ref, Sw, Hw), f"fused beside the unfused chain {mode} {shape}")
    finally:
        ar.release()
