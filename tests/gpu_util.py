"""Helpers for the -m gpu tests: call libdptx.so op entry points on torch CUDA tensors."""
import numpy as np
import torch

from omnidata_amd.engine import load_library, DTYPES

TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
# max |err| allowed relative to max |ref| when the OUTPUT is rounded to the 16-bit type
# (half an ulp of the largest value = 2^-9 / 2^-12, plus fp32 accumulation-order noise)
OUT_TOL = {"bf16": 6e-3, "fp16": 8e-4}


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def rel_err(a, ref):
    a, ref = a.double(), ref.double()
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-12))


def ulps(a, b):
    """fp32 ulp distance elementwise (-0 = +0; NaN = NaN)"""
    def ordered(x):
        i = np.ascontiguousarray(torch.as_tensor(x).float().cpu().numpy()).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    a32, b32 = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    d = np.abs(ordered(a32) - ordered(b32))
    both_nan = (torch.isnan(a32) & torch.isnan(b32)).numpy()
    return np.where(both_nan, 0, d)


def smooth(gen, B, H, W, lo, hi, k=5):
    """[B, 1, H, W] fp32 (CPU): a k x k grid of uniform draws interpolated to H x W, stretched to [lo, hi] per image"""
    g = torch.rand(B, 1, k, k, generator=gen)
    f = torch.nn.functional.interpolate(g, size=(H, W), mode="bilinear", align_corners=True)
    f = (f - f.amin((2, 3), keepdim=True)) / (f.amax((2, 3), keepdim=True) - f.amin((2, 3), keepdim=True)).clamp_min(1e-12)
    return (lo + (hi - lo) * f).float().contiguous()


def op_gemm(dtype, A, W, bias=None, R=None, act=0, c_fp32=False):
    lib = load_library()
    M, K = A.shape
    N = W.shape[0]
    C = torch.empty(M, N, device=A.device, dtype=torch.float32 if c_fp32 else TDT[dtype])
    rc = lib.dptx_op_gemm(DTYPES[dtype], ptr(A), ptr(W), ptr(bias), ptr(R), ptr(C), M, N, K, act,
                          int(A.dtype == torch.float32), int(c_fp32), int(R is not None and R.dtype == torch.float32), stream())
    assert rc == 0, rc
    return C


def op_conv(dtype, X, Wt, bias, R, stride, pad_t, pad_l, Ho, Wo, a_relu=0, act=0):
    """X NHWC [B,H,W,Cin]; Wt [Cout,k,k,Cin]."""
    lib = load_library()
    B, H, W, Cin = X.shape
    Cout, k = Wt.shape[0], Wt.shape[1]
    Y = torch.empty(B, Ho, Wo, Cout, device=X.device, dtype=TDT[dtype])
    rc = lib.dptx_op_conv(DTYPES[dtype], ptr(X), ptr(Wt), ptr(bias), ptr(R), ptr(Y), B, H, W, Cin, Cout, k, stride,
                          pad_t, pad_l, Ho, Wo, a_relu, act, stream())
    assert rc == 0, rc
    return Y


class PlaneArena:
    """bf16x3 / fp16x3 test storage: every tensor is a (hi, lo) pair of 16-bit planes a fixed distance apart,
    exactly like the engine's arena/blob halves."""

    def __init__(self, total_elems, device="cuda:0", dtype=torch.bfloat16):
        total_elems = (total_elems + 4095) // 4096 * 4096
        self.dtype = dtype
        self.buf = torch.zeros(2, total_elems, dtype=dtype, device=device)
        self.total, self.off = total_elems, 0
        load_library().dptx_op_set_planes(total_elems, total_elems)

    def _take(self, n):
        o = self.off
        self.off += (n + 127) // 128 * 128
        assert self.off <= self.total
        return o

    def put(self, t):
        t = t.float().to(self.buf.device)
        o = self._take(t.numel())
        hi = t.to(self.dtype)
        self.buf[0, o:o + t.numel()] = hi.flatten()
        self.buf[1, o:o + t.numel()] = (t - hi.float()).to(self.dtype).flatten()
        return self.buf[0, o:o + t.numel()].view(t.shape)

    def empty(self, *shape):
        n = 1
        for s in shape:
            n *= s
        o = self._take(n)
        return self.buf[0, o:o + n].view(*shape)

    def value(self, hi_view):
        """fp64 value hi + lo of a tensor handed out by put()/empty()."""
        o = hi_view.data_ptr() - self.buf.data_ptr()
        assert o % 2 == 0
        o //= 2
        n = hi_view.numel()
        return (self.buf[0, o:o + n].double() + self.buf[1, o:o + n].double()).view(hi_view.shape)

    def lo(self, hi_view):
        """the lo plane of a tensor handed out by put()/empty(), as a view of the same shape."""
        o = (hi_view.data_ptr() - self.buf.data_ptr()) // 2
        return self.buf[1, o:o + hi_view.numel()].view(hi_view.shape)

    def release(self):
        load_library().dptx_op_set_planes(0, 0)


# ------------------------------------------------------------------ inputs whose statistics differ row by row / group by group
# Normalisation kernels that apply one row's (group's, image's) statistics to another pass on inputs whose statistics are the
# same everywhere: the output moves by less than the 16-bit tolerance.  These generators give every row and every (image,
# group) pair statistics of its own, so that any such mix-up moves the output by many tolerances.  CPU tensors, fp32 (rows)
# or fp64 (NHWC); deterministic in `seed`.

def rows_with_stats(M, C, r_values=(0.0, 1.0, 8.0), outliers=False, near_constant=True, seed=0):
    """x [M, C] fp32 with statistics of its own in every row, and r = |mean| / std of every row (fp64, measured on x).

    Row m: a standardised Gaussian scaled by sigma_m = 2^e_m, e_m = (7 m mod 13) - 6 +- 1/4 (over [-6, 6], not monotonic;
    adjacent rows differ by a factor of 2^5.5 at least), plus mean_m = +-r_m sigma_m with r_m cycling through `r_values`.  outliers: 1-4 channels of every row then sit at
    30-300 sigma_m (either sign).  near_constant: row M // 2 becomes mean 3, sigma 3e-3 (r = 1000) without outliers.
    max |x| < 2^6.25 (max r + 300): inside fp16 for max r <= 64."""
    g = torch.Generator().manual_seed(seed)
    e = (7 * torch.arange(M) % 13 - 6).double() + 0.5 * torch.rand(M, generator=g, dtype=torch.float64) - 0.25
    sigma = torch.exp2(e)
    r = torch.tensor(r_values, dtype=torch.float64)[torch.arange(M) % len(r_values)]
    sign = torch.where(torch.rand(M, generator=g) < 0.5, -1.0, 1.0).double()
    z = torch.randn(M, C, generator=g, dtype=torch.float64)
    z = (z - z.mean(1, keepdim=True)) / z.std(1, unbiased=False, keepdim=True)
    if outliers:
        for m in range(M):
            k = int(torch.randint(1, 5, (1,), generator=g))
            ch = torch.randperm(C, generator=g)[:k]
            z[m, ch] = (30.0 + 270.0 * torch.rand(k, generator=g, dtype=torch.float64)) * torch.where(
                torch.rand(k, generator=g) < 0.5, -1.0, 1.0).double()
    if near_constant:
        m = M // 2
        z[m] = torch.randn(C, generator=g, dtype=torch.float64)
        sigma[m], r[m], sign[m] = 3e-3, 1000.0, 1.0
    x = ((sign * r * sigma).unsqueeze(1) + sigma.unsqueeze(1) * z).float()
    xd = x.double()
    return x, xd.mean(1).abs() / xd.std(1, unbiased=False)


def nhwc_with_group_stats(B, HW, C, groups=32, seed=0):
    """X [B, HW, C] fp64 with statistics of its own for every (image, group) pair of GroupNorm(groups).

    sigma[b, g] = 2^((5 g + 3 b) % 7 - 3): any two adjacent groups, and the same group of adjacent images, differ by a factor
    of 2 at least (5 and 3 are nonzero mod 7).  mean[b, g] = (-1)^(g + b) 1.5 sigma[b, g]: adjacent means have opposite signs,
    so they lie 1.5 (sigma + sigma') apart.  Values within 2^3 * 6 of zero: inside fp16 and its hi / lo planes."""
    g = torch.Generator().manual_seed(seed)
    cpg = C // groups
    gi = torch.arange(groups).view(1, groups)
    bi = torch.arange(B).view(B, 1)
    sigma = torch.exp2(((5 * gi + 3 * bi) % 7 - 3).double())                  # [B, G]
    mean = torch.where((gi + bi) % 2 == 0, 1.5, -1.5).double() * sigma
    z = torch.randn(B, HW, groups, cpg, generator=g, dtype=torch.float64).clamp(-4.0, 4.0)
    x = mean.view(B, 1, groups, 1) + sigma.view(B, 1, groups, 1) * z
    return x.reshape(B, HW, C)


def group_max(t, groups=32):
    """max |t| of every (image, group) of an NHWC [B, ..., C] tensor -> [B, groups] (fp64)."""
    B, C = t.shape[0], t.shape[-1]
    return t.double().abs().reshape(B, -1, groups, C // groups).transpose(1, 2).reshape(B, groups, -1).amax(-1)


def per_group_err(got, ref, groups=32, scale=None):
    """max |got - ref| / scale of every (image, group) of NHWC [B, ..., C] tensors -> [B, groups] (fp64); scale [B, groups]
    defaults to the group's max |ref|.  Behind a ReLU, pass the group's scale BEFORE the ReLU: a group the ReLU clips almost
    to zero keeps the absolute rounding of its pre-activation."""
    d = group_max(got.double() - ref.double(), groups)
    return d / (group_max(ref, groups) if scale is None else scale).clamp_min(1e-30)


def per_row_err(got, ref):
    """max |got - ref| / max |ref| of every row of [M, N] tensors -> [M] (fp64)."""
    d = (got.double() - ref.double()).abs().amax(-1)
    return d / ref.double().abs().amax(-1).clamp_min(1e-30)


# ------------------------------------------------------------------ attention, judged row by row
# One error number per tensor (rel_err) lets the rows that average many keys -- outputs 10-30x smaller than those of rows that
# look at one spiked key -- be wrong by tens of percent.  The helpers below give inputs in which every key counts, an fp64
# reference with the quantities a per-element bound needs, and that bound.  Pure torch, any device.

ATT_MODES = ("bf16", "fp16", "bf16x3", "fp16x3")
ATT_FAMILIES = ("flat", "peaked", "lastkeys")
ATT_SHAPES = ((2, 577, 12), (1, 505, 16), (1, 321, 16), (3, 129, 16), (1, 128, 12), (1, 193, 12), (3, 65, 12), (2, 17, 16),
              (1, 2, 12), (1, 1, 12))
ATT_PLANES = {"bf16": (torch.bfloat16, 1), "fp16": (torch.float16, 1), "bf16x3": (torch.bfloat16, 2), "fp16x3": (torch.float16, 2)}
ATT_U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "bf16x3": 2.0 ** -8, "fp16x3": 2.0 ** -11}
# fp32 floor of the plane modes: the largest |err| / A of tests/test_attention_host.py's model with P and the output left in fp32
# (no 16-bit rounding anywhere behind the operands), against attention_ref64, over ATT_SHAPES x ATT_FAMILIES x the two plane
# modes on a CPU.  It was measured against the reference, never against the kernel; test_fp32_floor_is_what_the_bound_uses
# re-measures it.
ATT_F32_FLOOR_MEASURED = 5.9e-6
ATT_F32_FLOOR_FACTOR = 4.0   # v_exp_f32 and the MFMA's accumulation order differ from torch's on the CPU


def attention_inputs(B, S, H, family, seed=0):
    """qkv [B, S, 3, H, 64] fp32 (CPU), deterministic in `seed`; b, h, s = image, head and token index.

    flat      Q x 2^-3: the softmax is near uniform, so every key carries about 1 / S of the output.
              V = 0.25 N(0, 1) + sign (1 + 0.25 ((h + b) % 5)), sign = +1 for even h + b, else -1: one key too many or too few
              moves every output by ~|v| / S, and neighbouring heads and images differ in sign and size.
    peaked    Q x 2^(0.5 ((5 h + 3 b) % 5)); V x vs + ((s + h) % 3 - 1) vs with vs = 2^((7 s + 3 h + b) % 9 - 4): every
              (image, head) has a temperature and every key a value scale of its own.
    lastkeys  K x (1 + 3 s / S), V + (s % 7 - 3): the running max grows in every tile and the last keys win.
    All values fit fp16 (asserted)."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(B, S, 3, H, 64, generator=g)
    b = torch.arange(B).view(B, 1, 1, 1)
    s = torch.arange(S).view(1, S, 1, 1)
    h = torch.arange(H).view(1, 1, H, 1)
    if family == "flat":
        x[:, :, 0] *= 2.0 ** -3
        sign = torch.where((h + b) % 2 == 0, 1.0, -1.0)
        x[:, :, 2] = 0.25 * x[:, :, 2] + sign * (1.0 + 0.25 * ((h + b) % 5))
    elif family == "peaked":
        x[:, :, 0] *= torch.exp2(0.5 * ((5 * h + 3 * b) % 5))
        vs = torch.exp2(((7 * s + 3 * h + b) % 9 - 4).float())
        x[:, :, 2] = x[:, :, 2] * vs + ((s + h) % 3 - 1) * vs
    elif family == "lastkeys":
        x[:, :, 1] *= 1.0 + 3.0 * s / S
        x[:, :, 2] += (s % 7 - 3).float()
    else:
        raise ValueError(family)
    assert float(x.abs().max()) < 60000.0
    return x.contiguous()


def attention_ref64(x):
    """fp64 attention of qkv values x [B, S, 3, H, 64] (the ROUNDED operands: hi + lo for the plane modes, PlaneArena.value).
    Returns o, A, l, Vsum, each broadcastable to the output layout [B, S, H, 64]:
      o    = softmax(Q K^T / 8) V
      A    = softmax(Q K^T / 8) |V|            the scale of every rounding that is relative to a term of the sum
      l    = 1 / max_j softmax  [B, S, H, 1]   the softmax denominator in the kernel's units (largest p = 1)
      Vsum = sum_j |v_j|        [B, 1, H, 64]
    Asserts max |logit log2 e| <= 64, which attention_row_bound's exponent-argument term assumes."""
    x = x.double()
    q, k, v = [t.permute(0, 2, 1, 3) for t in x.unbind(2)]          # [B, H, S, 64]
    logit = (q @ k.transpose(-1, -2)) * 0.125
    assert float(logit.abs().max()) * 1.4426950408889634 <= 64.0
    p = logit.softmax(-1)
    o = (p @ v).permute(0, 2, 1, 3)
    A = (p @ v.abs()).permute(0, 2, 1, 3)
    l = (1.0 / p.amax(-1, keepdim=True)).permute(0, 2, 1, 3)
    Vsum = v.abs().sum(2, keepdim=True).permute(0, 2, 1, 3)
    return o, A, l, Vsum


def attention_row_bound(mode, A, l, Vsum):
    """Elementwise bar on |out - o| of the attention kernel, u = 2^-8 (bf16) / 2^-11 (fp16) the unit roundoff.

    bf16, fp16:      (2 u + 2^-17) A  [+ 2^-25 Vsum / l for fp16]
        u A       P is rounded to 16 bit before the PV product
        u A       the output is rounded to 16 bit (u |o| <= u A)
        2^-17 A   fp32: the rounding of the exponent's argument, ln 2 * 3 * Lmax * 2^-24 with Lmax <= 64 (attention_ref64
                  asserts it), and the accumulation
        2^-25 Vsum / l   an fp16 P below 2^-14 is subnormal: absolute error 2^-25 per key, in the running scale, which never
                  exceeds the final one (l)
    bf16x3, fp16x3:  (3 u^2 + f32) A  [+ 2^-25 Vsum / l for fp16x3]
        3 u^2     the hi / lo split of P, the dropped lo * lo products, the hi / lo split of the output
        f32       4 x 5.9e-6 = 2.36e-5 (ATT_F32_FLOOR_FACTOR x ATT_F32_FLOOR_MEASURED): the fp32 floor depends on exp2 and on
                  the accumulation order and has no tight derivation; 5.9e-6 is the largest |err| / A (5.81e-6, fp16x3 lastkeys
                  2x577x12, rounded up) of the CPU model with nothing rounded to 16 bit behind the operands, against
                  attention_ref64, over the whole test matrix -- measured against the reference, not against the kernel; the
                  factor 4 is there because the GPU's v_exp_f32 and the MFMA's accumulation order differ from torch's on a
                  CPU (profiles/attention_rows.md)."""
    u = ATT_U[mode]
    if ATT_PLANES[mode][1] == 1:
        bound = (2.0 * u + 2.0 ** -17) * A
    else:
        bound = (3.0 * u * u + ATT_F32_FLOOR_FACTOR * ATT_F32_FLOOR_MEASURED) * A
    if ATT_PLANES[mode][0] == torch.float16:
        bound = bound + 2.0 ** -25 * Vsum / l
    return bound


def attention_planes(x, mode):
    """(hi, lo) 16-bit planes of fp32 values x as PlaneArena.put splits them; lo is None for the single-plane modes."""
    dt, pl = ATT_PLANES[mode]
    hi = x.float().to(dt)
    return hi, ((x.float() - hi.float()).to(dt) if pl == 2 else None)


# ------------------------------------------------------------------ GEMMs and convolutions, judged element by element
# One error number per tensor (rel_err against max |ref|) lets a store that truncates instead of rounding pass (2^-7 |y| is
# 3.9e-3 of the largest element, under the 6e-3 bar), and lets every row 100x smaller than the largest be wholly wrong.  The
# helpers below give operands whose rows and columns carry scales of their own, an fp64 reference together with the magnitude
# sum S that an accumulation error is relative to, and the bar on every single element.  Pure torch, any device.

GEMM_MODES = ATT_MODES
GEMM_PLANES = ATT_PLANES
GEMM_U = ATT_U
# fp32 floor: the largest |y32 - y| / S over (300, 64, 64), (515, 256, 768), (260, 128, 3072), (200, 256, 6912) x {bf16, fp16}
# operands of scaled_gemm_operands (seed 0), y32 = A W^T + bias + R evaluated in plain fp32 on a CPU, y and S from gemm_ref64.
# The largest was fp16 at (300, 64, 64): 1.65e-7 with these operands, 1.8e-7 with another draw of the same family -- the
# constant is the larger; every K from 64 to 6912 lay between 5e-8 and that.  Measured against the reference, never against
# a kernel; tests/test_gemm_bound_host.py re-measures it (profiles/gemm_elements.md).
GEMM_F32_FLOOR_MEASURED = 1.8e-7
GEMM_F32_FLOOR_FACTOR = 4.0   # the MFMA's accumulation order differs from a CPU's (attention uses the same margin)
GEMM_HOST_SHAPES = ((300, 64, 64), (515, 256, 768), (260, 128, 3072), (200, 256, 6912))


def _row_exp(n):
    """e_m = (7 m mod 13) - 6 for m < n: over [-6, 6], adjacent values differ by 7 or 6."""
    return ((7 * torch.arange(n)) % 13 - 6).double()


def _col_exp(n):
    """f_n = (5 n mod 7) - 3 for n < n: over [-3, 3], adjacent values differ by 5 or 2."""
    return ((5 * torch.arange(n)) % 7 - 3).double()


def scaled_gemm_operands(M, N, K, seed=0):
    """A [M, K], W [N, K], bias [N], R [M, N] in fp64 (CPU), deterministic in `seed`: the caller rounds them to the type or
    splits them into planes (PlaneArena.put).
      A[m, :] = 2^e_m N(0, 1), e_m = (7 m mod 13) - 6;  W[n, :] = K^-1/2 2^f_n N(0, 1), f_n = (5 n mod 7) - 3;
      bias[n] = 2^f_n N(0, 1);  R[m, n] = 2^(e_m + f_n) N(0, 1).
    Adjacent rows and adjacent columns differ in scale by 2^2 at least.  max |A W^T + bias + R| < 60000 (asserted; ~2.8e3)."""
    g = torch.Generator().manual_seed(2000 + seed)
    se, sf = torch.exp2(_row_exp(M)), torch.exp2(_col_exp(N))
    A = torch.randn(M, K, generator=g, dtype=torch.float64) * se[:, None]
    W = torch.randn(N, K, generator=g, dtype=torch.float64) * sf[:, None] * K ** -0.5
    bias = torch.randn(N, generator=g, dtype=torch.float64) * sf
    R = torch.randn(M, N, generator=g, dtype=torch.float64) * se[:, None] * sf[None, :]
    assert float((A @ W.t() + bias + R).abs().max()) < 60000.0
    return A, W, bias, R


def scaled_conv_operands(B, H, W, Cin, Cout, k, seed=0, Ho=None, Wo=None):
    """X [B, H, W, Cin] NHWC, Wt [Cout, k, k, Cin], bias [Cout], R [B, Ho, Wo, Cout] (Ho, Wo default to H, W) in fp64 (CPU).
    The scale of X[b, y, x, :] follows the flat pixel index p over the whole batch, 2^((7 p mod 13) - 6); weight rows and the
    bias follow f_n with K = k k Cin; R follows (flat output pixel) x channel.  |values| < 2^6 * 6 sigma: inside fp16."""
    g = torch.Generator().manual_seed(3000 + seed)
    Ho, Wo = H if Ho is None else Ho, W if Wo is None else Wo
    sf = torch.exp2(_col_exp(Cout))
    X = torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64) * torch.exp2(_row_exp(B * H * W)).view(B, H, W, 1)
    Wt = torch.randn(Cout, k, k, Cin, generator=g, dtype=torch.float64) * sf.view(-1, 1, 1, 1) * (k * k * Cin) ** -0.5
    bias = torch.randn(Cout, generator=g, dtype=torch.float64) * sf
    R = torch.randn(B, Ho, Wo, Cout, generator=g, dtype=torch.float64) * torch.exp2(_row_exp(B * Ho * Wo)).view(B, Ho, Wo, 1) * sf
    return X, Wt, bias, R


def gemm_operand_planes(x, mode):
    """(hi, lo) 16-bit planes of values x as PlaneArena.put splits them (through fp32); lo is None for the one-plane modes."""
    return attention_planes(x, mode)


def epilogue_ref64(acc, Sacc, bias, R, act):
    """y = act(acc + bias) + R and S = Sacc + |bias| + |R| (fp64); act 0 none, 1 ReLU, 2 erf-GELU."""
    y, S = acc, Sacc
    if bias is not None:
        y, S = y + bias.double(), S + bias.double().abs()
    if act == 1:
        y = torch.relu(y)
    elif act == 2:
        y = torch.nn.functional.gelu(y)
    if R is not None:
        y, S = y + R.double(), S + R.double().abs()
    return y, S


def gemm_ref64(A, W, bias=None, R=None, act=0):
    """fp64 (y, S) of the values the kernel reads (hi + lo for the plane modes, the hi plane where only that is read):
    y = act(A W^T + bias) + R, the final value; S = sum_k |a_k| |w_k| + |bias| + |R|, what a rounding of any term of the sum is
    relative to."""
    A, W = A.double(), W.double()
    return epilogue_ref64(A @ W.t(), A.abs() @ W.abs().t(), bias, R, act)


def conv_acc64(X, Wt, stride=1, pad_t=0, pad_l=0, Ho=None, Wo=None, a_relu=0):
    """(conv(x', w), conv(|x'|, |w|)) in fp64, NHWC: X [B, H, W, Cin], Wt [Cout, k, k, Cin], zero padding pad_t rows above and
    pad_l columns left, below and right whatever (Ho, Wo) leave over, x' = relu(x) when a_relu.  One matrix product per tap:
    no backend's convolution is involved."""
    X, Wt = X.double(), Wt.double()
    if a_relu:
        X = torch.relu(X)
    B, H, W_, Cin = X.shape
    Cout, k = Wt.shape[0], Wt.shape[1]
    Ho = (H + 2 * pad_t - k) // stride + 1 if Ho is None else Ho
    Wo = (W_ + 2 * pad_l - k) // stride + 1 if Wo is None else Wo
    pb = max((Ho - 1) * stride + k - H - pad_t, 0)
    pr = max((Wo - 1) * stride + k - W_ - pad_l, 0)
    Xp = torch.nn.functional.pad(X, [0, 0, pad_l, pr, pad_t, pb])
    assert Xp.shape[1] >= (Ho - 1) * stride + k and Xp.shape[2] >= (Wo - 1) * stride + k
    acc = torch.zeros(B, Ho, Wo, Cout, dtype=torch.float64, device=X.device)
    Sacc = torch.zeros_like(acc)
    for ky in range(k):
        for kx in range(k):
            win = Xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride, :]
            w = Wt[:, ky, kx, :].t()
            acc += win @ w
            Sacc += win.abs() @ w.abs()
    return acc, Sacc


def conv_ref64(X, Wt, bias=None, R=None, stride=1, pad_t=0, pad_l=0, Ho=None, Wo=None, a_relu=0, act=0):
    """fp64 (y, S) of an NHWC convolution of the values the kernel reads (conv_acc64 has the geometry):
    y = act(conv(x', w) + bias) + R [B, Ho, Wo, Cout], S = conv(|x'|, |w|) + |bias| + |R|."""
    return epilogue_ref64(*conv_acc64(X, Wt, stride, pad_t, pad_l, Ho, Wo, a_relu), bias, R, act)


def gemm_elem_bound(mode, y, S, act, c_fp32=False, planes=None, floor_measured=None):
    """Elementwise bar on |got - y| of a GEMM / convolution output; u = 2^-8 (bf16) / 2^-11 (fp16) the unit roundoff and
    F = GEMM_F32_FLOOR_FACTOR x GEMM_F32_FLOOR_MEASURED = 7.2e-7 the fp32 floor (accumulation order, bias and residual adds).

      one 16-bit plane       u |y| + F S      the stored value is the nearest 16-bit number
      fp32 (c_fp32)          F S              (u^2 + F) S in the plane modes: their product drops lo * lo, at most u^2 |a| |w|
                                              per term, whatever the output's type; nothing is split
      hi / lo pair           (3 u^2 + F) S    the dropped lo * lo products, the split of the output, one spare
      any fp16 plane         + 2^-25          a plane value below 2^-14 is subnormal
      act == 2               F S -> 1.13 F S + 2e-6    1.13 = max |gelu'|; 2e-6 = twice the absolute error that
                                                       tests/test_gelu_formula.py pins for the device formula
    ReLU is 1-Lipschitz and changes nothing.  planes: how many planes the OUTPUT has where that is not the mode's own count
    (the epi2 forms write a pair from a one-plane product; c_hi_only writes one plane from a two-plane kernel).
    floor_measured: the measured fp32 floor where the kernel has one of its own (the stem: STEM_F32_FLOOR_MEASURED)."""
    dt, pl = GEMM_PLANES[mode]
    pl = pl if planes is None else planes
    u = GEMM_U[mode]
    F = GEMM_F32_FLOOR_FACTOR * (GEMM_F32_FLOOR_MEASURED if floor_measured is None else floor_measured)
    floor = 1.13 * F * S + 2e-6 if act == 2 else F * S
    if c_fp32:
        return floor + u * u * S if GEMM_PLANES[mode][1] == 2 else floor
    bound =u * y.abs() + floor if pl == 1 else 3.0 * u * u * S + floor
    if dt == torch.float16:
        bound = bound + 2.0 ** -25
    return bound


def elements_outside(got, y, bound):
    """(worst |got - y| / bound, indices of the first five elements outside the bound -- a NaN is outside)."""
    err = (got.double() - y).abs()
    bad = ~(err <= bound)
    worst = float((err / bound).nan_to_num(nan=float("inf")).max())
    return worst, torch.nonzero(bad)[:5].tolist()


def assert_elements_inside(got, y, bound, what):
    """Every element of `got` within `bound` of y: prints the worst |err| / bound, and on failure the first offending
    (row, column) / (image, y, x, channel) indices.  Returns the worst ratio."""
    worst, bad = elements_outside(got, y, bound)
    print(f"\n[elements] {what}: worst |err| / bound {worst:.3f}")
    assert not bad, f"{what}: worst |err| / bound {worst:.3f}, first elements outside {bad}"
    return worst


# ------------------------------------------------------------------ the kernels that interpolate, judged element by element
# The x2 up-sampling (csrc/misc.hip) and the fused head tail (csrc/head.hip) against fp64.  rel_err lets a wrong value in a
# small channel, a wrong halo column at a tile seam and a flipped 16-bit rounding in the window pass; the helpers below give
# operands with a scale of their own in every pixel and channel, fp64 references with the magnitude sums a bound is relative
# to, and the bars on every single element.  Pure torch, any device.  tests/test_head_bound_host.py shows on a CPU which
# mistakes the bars reject; profiles/head_elements.md has the figures.

UP_VARIANTS = ("y:sub x:sub", "y:sub x:fma", "y:fma x:sub", "y:fma x:fma")
# fp32 floor of the blend in units of 2^-24 Sb: the largest |F.interpolate(fp32) - upsample_ref64| / (2^-24 Sb) on a CPU over
# UP_HOST_CASES x the four modes' operands (scaled_head_operands, seed 0), each case against the variant that fits it best
# (on a CPU always "y:sub x:sub").  The sixteen figures lay between 2.87 and 4.43, the largest bf16x3 at (1, 96, 96, 128) -- the
# roundings of 1 - l1 on either axis, of six products and of three sums.  Measured against the reference, never against a
# kernel; tests/test_head_bound_host.py re-measures it (profiles/head_elements.md).
UP_F32_FLOOR_MEASURED = 4.5
UP_HOST_CASES = ((1, 4, 16, 128), (2, 12, 16, 128), (3, 20, 48, 128), (1, 96, 96, 128))
HEAD_HOST_SHAPES = ((1, 4, 16, 1, 1), (2, 4, 32, 3, 0), (2, 12, 16, 2, 1), (3, 20, 48, 3, 1))


def scaled_head_operands(B, Hs, Ws, C, seed=0, Cin=128):
    """H0 [B, Hs, Ws, Cin], W2 [32, 3, 3, Cin], b2 [32], w4 [C, 32], b4 [C] in fp64 (CPU), deterministic in `seed`.
      H0[b, y, x, c] = 2^((7 p mod 13) - 6) 2^((5 c mod 7) - 3) N(0, 1), p the flat pixel index over the batch: the family of
      scaled_conv_operands with a scale per channel on top;  W2[n], b2[n] carry 2^((5 n mod 7) - 3) as there (K = 9 Cin);
      w4[c, :] = (8, 1, 1/8, 1)[c] 32^-1/2 N(0, 1) and b4[c] = (8, 1, 1/8, 1)[c] N(0, 1): a small output channel is judged by
      its own size.  |H0| < 2^9 * 6: inside fp16."""
    g = torch.Generator().manual_seed(4000 + seed)
    H0 = (torch.randn(B, Hs, Ws, Cin, generator=g, dtype=torch.float64) * torch.exp2(_row_exp(B * Hs * Ws)).view(B, Hs, Ws, 1)
          * torch.exp2(_col_exp(Cin)))
    sf = torch.exp2(_col_exp(32))
    W2 = torch.randn(32, 3, 3, Cin, generator=g, dtype=torch.float64) * sf.view(-1, 1, 1, 1) * (9 * Cin) ** -0.5
    b2 = torch.randn(32, generator=g, dtype=torch.float64) * sf
    rs = torch.tensor([8.0, 1.0, 0.125, 1.0], dtype=torch.float64)[:C]
    w4 = torch.randn(C, 32, generator=g, dtype=torch.float64) * rs[:, None] * 32 ** -0.5
    b4 = torch.randn(C, generator=g, dtype=torch.float64) * rs
    return H0, W2, b2, w4, b4


def up_axis32(n_in, variant_fma, device="cpu"):
    """(i0, i1, l0, l1) of one axis of the x2 align-corners up-sampling in ATen's fp32 formulation: ratio = (in - 1) / (out - 1),
    src = ratio dst, i0 = int(src), i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1, everything rounded to fp32.  l1 has two
    legitimate values: fl32(fl32(ratio dst) - i0) (variant_fma False: the subtraction itself is exact) and fl32(ratio dst - i0)
    with the product not rounded (True: what a compiler's fma contraction gives; exact to form in fp64, where the product of
    two fp32 numbers and its difference to a small integer are representable).  i0 comes from the rounded product either way."""
    n_out = 2 * n_in
    ratio = (torch.tensor(float(n_in - 1), dtype=torch.float32) / torch.tensor(float(n_out - 1), dtype=torch.float32))
    dst = torch.arange(n_out, dtype=torch.float32)
    src = ratio * dst                                        # fp32, rounded
    i0 = src.to(torch.int64)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    if variant_fma:
        l1 = (ratio.double() * dst.double() - i0.double()).float()
    else:
        l1 = src - i0.float()
    l0 = 1.0 - l1                                            # fp32, rounded
    return i0.to(device), i1.to(device), l0.to(device), l1.to(device)


def upsample_ref64(X, variant):
    """(y, Sb) in fp64 of the x2 bilinear align-corners up-sampling of the values X [B, H, W, C] the kernel reads (hi + lo for
    the plane modes): indices and weights in fp32 (up_axis32; variant 0..3 = UP_VARIANTS picks how l1 is rounded on the two
    axes), the blend ly0 (lx0 a + lx1 b) + ly1 (lx0 c + lx1 d) in fp64.  Sb is the same blend of |values| with |weights|: what
    a rounding of any weight, product or partial sum is relative to."""
    X = X.double()
    y0, y1, ly0, ly1 = up_axis32(X.shape[1], bool(variant & 2), X.device)
    x0, x1, lx0, lx1 = up_axis32(X.shape[2], bool(variant & 1), X.device)
    ly0, ly1 = ly0.double().view(1, -1, 1, 1), ly1.double().view(1, -1, 1, 1)
    lx0, lx1 = lx0.double().view(1, 1, -1, 1), lx1.double().view(1, 1, -1, 1)
    r0, r1 = X[:, y0], X[:, y1]
    a, b, c, d = r0[:, :, x0], r0[:, :, x1], r1[:, :, x0], r1[:, :, x1]
    y = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)
    Sb = ly0.abs() * (lx0.abs() * a.abs() + lx1.abs() * b.abs()) + ly1.abs() * (lx0.abs() * c.abs() + lx1.abs() * d.abs())
    return y, Sb


def up_elem_bound(mode, y, Sb):
    """Elementwise bar on |got - y| of the up-sampling; u the unit roundoff of the plane type and c = GEMM_F32_FLOOR_FACTOR x
    UP_F32_FLOOR_MEASURED = 18 the fp32 floor of the blend in units of 2^-24 Sb (measured on a CPU, see the constant).

      one 16-bit plane    u |y| + c 2^-24 Sb       the stored value is the nearest 16-bit number to the fp32 blend
      hi / lo pair        (3 u^2 + c 2^-24) Sb     the split of the output (u^2 |y| <= u^2 Sb), two spare
      any fp16 plane      + 2^-25                  a plane value below 2^-14 is subnormal
    A launch passes when ALL its elements are inside the bar for ONE of the four variants of upsample_ref64: a kernel uses one
    arithmetic throughout."""
    dt, pl = GEMM_PLANES[mode]
    u = GEMM_U[mode]
    floor = GEMM_F32_FLOOR_FACTOR * UP_F32_FLOOR_MEASURED * 2.0 ** -24 * Sb
    bound = u * y.abs() + floor if pl == 1 else 3.0 * u * u * Sb + floor
    if dt == torch.float16:
        bound = bound + 2.0 ** -25
    return bound


def upsample_variants_inside(got, X, mode):
    """{variant index: worst |err| / bound} of `got` against upsample_ref64(X, variant) / up_elem_bound for the four variants,
    and the set of variants for which every element is inside."""
    worst, inside = {}, set()
    for v in range(4):
        y, Sb = upsample_ref64(X, v)
        w, bad = elements_outside(got, y, up_elem_bound(mode, y, Sb))
        worst[v] = w
        if not bad:
            inside.add(v)
    return worst, inside


def head_tail_ref64(U, W2, b2, w4, b4, relu):
    """fp64 reference of the head chain behind the up-sampling, from the up-sampled values U [B, Ho, Wo, 128] (NHWC):
      h = relu(conv3x3(U, W2, pad 1) + b2)    S_h = conv(|U|, |W2|) + |b2|    (conv_acc64: one matrix product per tap)
      y = w4 h + b4, relu(y) when `relu`
    Returns (y, Sw, Hw, Hh) in the kernel's NCHW layout [B, C, Ho, Wo]: Sw = sum_n |w4| S_h, what a rounding inside the
    convolution's sum is relative to once projected; Hw = sum_n |w4| |h| + |b4|, the same for the projection; Hh = sum_n |w4| |h|
    alone, what a rounding of the stored h is relative to."""
    W2, b2, w4, b4 = W2.double(), b2.double(), w4.double(), b4.double()
    acc, Sacc = conv_acc64(U, W2, 1, 1, 1)
    h = torch.relu(acc + b2)
    Sh = Sacc + b2.abs()
    y = h @ w4.t() + b4
    if relu:
        y = torch.relu(y)
    Sw = Sh @ w4.abs().t()
    Hh = h.abs() @ w4.abs().t()
    Hw = Hh + b4.abs()
    return y.permute(0, 3, 1, 2), Sw.permute(0, 3, 1, 2), Hw.permute(0, 3, 1, 2), Hh.permute(0, 3, 1, 2)


def head_elem_bound(mode, y, Sw, Hw, io=None, h_planes=0, Hh=None):
    """Elementwise bar on |got - y| of the head tail; F = GEMM_F32_FLOOR_FACTOR x GEMM_F32_FLOOR_MEASURED = 7.2e-7, u the unit
    roundoff of the plane type, (y, Sw, Hw, Hh) from head_tail_ref64.

      F (Sw + Hw)                 fp32: the convolution's accumulation and bias (relative to S_h, carried through |w4|; ReLU is
                                  1-Lipschitz) and the 32-term projection with its bias (relative to sum |w4| |h| + |b4|)
      + u^2 Sw                    plane modes: every product drops lo * lo, at most u^2 |U| |W2| per term
      + u_io |y|                  a 16-bit result (io = "bf16" / "fp16")
    The unfused chain stores h before the projection reads it (h_planes = 1 or 2), which the bias b4 has no part in:
      + u Hh                      one plane: sum |w4| u |h|
      + 3 u^2 Hh                  a pair: the split of h"""
    u = GEMM_U[mode]
    F = GEMM_F32_FLOOR_FACTOR * GEMM_F32_FLOOR_MEASURED
    bound = F * (Sw + Hw)
    if GEMM_PLANES[mode][1] == 2:
        bound = bound + u * u * Sw
    if h_planes == 1:
        bound = bound + u * Hh
    elif h_planes == 2:
        bound = bound + 3.0 * u * u * Hh
    if io in ("bf16", "fp16"):
        bound = bound + GEMM_U[io] * y.abs()
    return bound


def head_out_ref64(X, Xlo, w, b, relu):
    """(y, S) in fp64 of the 1x1 projection of x = X (+ Xlo, the lo plane, unless None) [B, HW, 32] -> NCHW [B, Cout, HW]:
    y = w x + b (ReLU when `relu`), S = sum |w| |x| + |b|.  Row blocks of 2^20 pixels: the largest test has 4.2 M of them."""
    w, b = w.double(), b.double()
    B, HW, _ = X.shape
    y = torch.empty(B, w.shape[0], HW, dtype=torch.float64, device=X.device)
    S = torch.empty_like(y)
    for i in range(0, HW, 1 << 20):
        x = X[:, i:i + (1 << 20)].double()
        if Xlo is not None:
            x = x + Xlo[:, i:i + (1 << 20)].double()
        v = x @ w.t() + b
        y[:, :, i:i + (1 << 20)] = (torch.relu(v) if relu else v).transpose(1, 2)
        S[:, :, i:i + (1 << 20)] = (x.abs() @ w.abs().t() + b.abs()).transpose(1, 2)
    return y, S


# ------------------------------------------------------------------ the stem and the glue kernels, judged element by element
# The stem convolution (csrc/stem.hip), GroupNorm (+ ReLU + max-pool) (csrc/norm.hip) and the position-embedding resize
# (csrc/misc.hip) against fp64.  One number per tensor, or per (image, group), lets a truncating store, a dropped window tap, a
# wrong value in a small channel or at a dim pixel pass; the helpers below give operands with a scale of their own per pixel
# and channel, fp64 references with the magnitude sums a bound is relative to, and the bars on every single element.  Pure
# torch, any device.  tests/test_stem_bound_host.py measures the floors and shows on a CPU which mistakes the bars reject;
# profiles/stem_elements.md has the figures.

STEM_SHAPES = ((1, 8, 8), (3, 16, 40), (1, 8, 256), (1, 16, 136), (2, 24, 264))                     # (B, H, W)
STEM_IO = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
POOL_SHAPES = ((1, 2, 2, 64), (2, 4, 6, 64), (3, 16, 24, 64), (1, 34, 30, 64), (2, 32, 48, 64), (1, 96, 96, 64),
               (2, 8, 8, 128))                                                                       # (B, H, W, C)
GN_ELEM_CASES = ((2, 100, 64, 1, False), (1, 33, 512, 1, False), (3, 300, 256, 0, True), (2, 40, 1024, 1, True),
                 (2, 2304, 128, 1, True))                                                            # (B, HW, C, relu, residual)
POS_GRIDS = ((12, 32), (1, 1), (40, 24), (64, 48), (23, 25))                                         # (gh, gw)
# fp32 floor of the stem: the largest |y32 - y| / S over STEM_SHAPES x the four modes x the three image types (stem_operands,
# seed 0), y32 the fp32 model of tests/test_stem_bound_host.py that accumulates in the kernel's order -- eleven k-steps of 16
# (two (c, ky) rows of 8 taps) in ascending order, one fp32 addition per MFMA -- with nothing rounded behind the operands, y and
# S from stem_ref64.  K is 147 and the accumulator takes eleven (33 in the plane modes) rounded additions of partial sums of
# either sign, which reads above the dense GEMM's 1.8e-7.  Measured against the reference, never against the kernel;
# test_stem_floor_is_what_the_bound_uses re-measures it.
STEM_F32_FLOOR_MEASURED = 3.2e-7
# fp32 floor of GroupNorm (+ ReLU + max-pool) in units of 2^-24 T: the largest |y32 - y| / (2^-24 T) over POOL_SHAPES and
# GN_ELEM_CASES x the four modes, y32 the fp32 model of tests/test_stem_bound_host.py -- fp32 (sum, sum of squares) per
# gn_chunks record, fp64 across the records, mean and rstd rounded to fp32, a = rstd gamma rounded, d = fma(-a, mean, beta),
# fma(x, a, d) --, y and T from gn_pool_ref64 / gn_ref64.  Measured against the reference, never against the kernel;
# test_gn_floor_is_what_the_bound_uses re-measures it.
GN_F32_FLOOR_MEASURED = 9.1
# fp32 error of a source coordinate of pos_resize_kernel, s = max((dst + 0.5) r - 0.5, 0) with r = fl(24 / g): three roundings.
# r carries 2^-24 relatively, which (dst + 0.5) r < 32 turns into 2^-19 at most; the product below 32 is rounded by half an
# ulp, 2^-20 at most; so is the difference (exact above 0.5).  2^-19 + 2^-20 + 2^-20 = 2^-18.  l1 = s - i0 is exact.
POS_COORD_ERR = 2.0 ** -18


def plane_value(p):
    """fp64 value of a (hi, lo) pair of gemm_operand_planes; lo may be None."""
    return p[0].double() if p[1] is None else p[0].double() + p[1].double()


def stem_operands(B, H, W, seed=0):
    """(x [B, 3, H, W] NCHW, wp [64, 176], X [B, H, W, 3] NHWC, Wt [64, 7, 7, 3] OHWI) in fp64 (CPU), deterministic in `seed`:
    scaled_conv_operands(B, H, W, 3, 64, 7, seed) -- every pixel carries 2^((7 p mod 13) - 6) and a sign per value, every
    output channel 2^((5 n mod 7) - 3).  x and X, wp and Wt hold the same values: x and wp are what the kernel takes (wp packed
    with k = (c 7 + ky) 8 + kx, zero in tap kx = 7 and in k >= 168), X and Wt what conv_ref64 takes."""
    X, Wt, _, _ = scaled_conv_operands(B, H, W, 3, 64, 7, seed)
    wp = torch.zeros(64, 176, dtype=torch.float64)
    wp[:, :168].view(64, 3, 7, 8)[..., :7] = Wt.permute(0, 3, 1, 2)
    return X.permute(0, 3, 1, 2).contiguous(), wp, X, Wt


def stem_image_planes(x, mode, io):
    """(hi, lo) planes of the image as the kernel forms them: the caller's values rounded to the image type `io` first, then
    rounded to the mode's plane type, or split hi = dt(x), lo = dt(x - hi) in the plane modes."""
    return gemm_operand_planes(x.float().to(STEM_IO[io]).float(), mode)


def stem_ref64(X, Wt, mode, io="fp32"):
    """fp64 (y, S) [B, H/2, W/2, 64] of the stem convolution of the values the MFMAs read: conv_ref64(x', w', stride 2, one
    matrix product per tap) with TF-SAME padding (2 above and left, 3 below and right), x' = the image X [B, H, W, 3] rounded
    to `io` and then to the plane type (hi + lo in the plane modes), w' = the weight Wt [64, 7, 7, 3] rounded or split the
    same way."""
    H, W = X.shape[1], X.shape[2]
    xv = plane_value(stem_image_planes(X, mode, io))
    wv = plane_value(gemm_operand_planes(Wt, mode))
    return conv_ref64(xv, wv, stride=2, pad_t=2, pad_l=2, Ho=H // 2, Wo=W // 2)


def stem_elem_bound(mode, y, S):
    """gemm_elem_bound with the stem's own fp32 floor F = GEMM_F32_FLOOR_FACTOR x STEM_F32_FLOOR_MEASURED:
    u |y| + F S (one plane), (3 u^2 + F) S (a pair), + 2^-25 with an fp16 plane."""
    return gemm_elem_bound(mode, y, S, 0, floor_measured=STEM_F32_FLOOR_MEASURED)


def pool_operands(B, H, W, C, seed=0):
    """X [B, H W, C] fp64 (CPU): nhwc_with_group_stats times 2^((3 p mod 5) - 2), p the flat pixel index over the batch, so
    that the taps of one pooling window differ in size (adjacent pixels by 2^3 or 2^2) and a dropped or misplaced tap moves
    the maximum.  |values| < 2^5 * 6: inside fp16."""
    X = nhwc_with_group_stats(B, H * W, C, seed=seed)
    f = torch.exp2(((3 * torch.arange(B * H * W)) % 5 - 2).double()).view(B, H * W, 1)
    return X * f


def gn_params(C, seed=0):
    """(gamma [C], beta [C]) fp32 (CPU) of either sign, deterministic in `seed`."""
    g = torch.Generator().manual_seed(5000 + seed)
    return torch.randn(C, generator=g), torch.randn(C, generator=g)


def gn_affine64(X, gamma, beta, eps, groups=32):
    """(a, d, mean) [B, 1, C] fp64 of GroupNorm(groups) of X [B, HW, C]: the biased statistics of every (image, group) in fp64,
    a = gamma rstd, d = beta - mean a, so that gn(x) = x a + d."""
    X = X.double()
    B, HW, C = X.shape
    cpg = C // groups
    xg = X.reshape(B, HW, groups, cpg)
    mean = xg.mean((1, 3))
    var = ((xg - mean.view(B, 1, groups, 1)) ** 2).mean((1, 3))
    rstd = 1.0 / torch.sqrt(var + eps)
    a = gamma.double().view(1, C) * rstd.repeat_interleave(cpg, 1)
    m = mean.repeat_interleave(cpg, 1)
    d = beta.double().view(1, C) - m * a
    return a.view(B, 1, C), d.view(B, 1, C), m.view(B, 1, C)


def window_max(v, H, W, y_from=0, size=3):
    """max over the window {2 o + y_from .. 2 o + y_from + size - 1}^2 within the image of v [B, H, W, C] -> [B, (H + 1) / 2,
    (W + 1) / 2, C]; taps outside the image count as -inf (MaxPool2dSame(3, 2) of an even size: y_from 0, size 3)."""
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    lead = -min(y_from, 0)
    vp = torch.nn.functional.pad(v, [0, 0, lead, 2 * Wo + size + 1, lead, 2 * Ho + size + 1], value=float("-inf"))
    out = None
    for dy in range(size):
        for dx in range(size):
            y0, x0 = dy + y_from + lead, dx + y_from + lead
            s = vp[:, y0:y0 + 2 * Ho - 1:2, x0:x0 + 2 * Wo - 1:2]
            out = s if out is None else torch.maximum(out, s)
    return out


def gn_ref64(X, gamma, beta, R=None, relu=0, eps=1e-5):
    """fp64 (y, T) [B, HW, C] of GroupNorm(32) (+ residual R, + ReLU) of the stored values X [B, HW, C] (hi + lo in the plane
    modes): y = relu(x a + d + R), T = |x| |a| + |mean| |a| + |beta| + |R|, what a rounding of the statistics, of the affine or
    of the sum is relative to."""
    X = X.double()
    a, d, m = gn_affine64(X, gamma, beta, eps)
    y = X * a + d
    T = X.abs() * a.abs() + m.abs() * a.abs() + beta.double().abs().view(1, 1, -1)
    if R is not None:
        y, T = y + R.double(), T + R.double().abs()
    return (torch.relu(y) if relu else y), T


def gn_pool_ref64(X, gamma, beta, H, W, eps=1e-5):
    """fp64 (y, T) [B, H/2, W/2, C] of the stem's GroupNorm(32) + ReLU + MaxPool2dSame(3, 2) of the stored values X [B, H W, C]:
    v = x a + d with the fp64 statistics of every (image, group); y = max(0, max of v over the window {2 oy .. 2 oy + 2} x
    {2 ox .. 2 ox + 2} within the image); T = max over the same window of |x| |a| + |mean| |a| + |beta|."""
    X = X.double()
    B, _, C = X.shape
    v, T = gn_ref64(X, gamma, beta, None, 0, eps)
    y = torch.relu(window_max(v.view(B, H, W, C), H, W))
    return y, window_max(T.view(B, H, W, C), H, W)


def gn_elem_bound(mode, y, T):
    """Elementwise bar on |got - y| of GroupNorm (+ ReLU + max-pool); u the unit roundoff of the plane type, (y, T) from
    gn_ref64 / gn_pool_ref64 and c = GEMM_F32_FLOOR_FACTOR x GN_F32_FLOOR_MEASURED the fp32 floor in units of 2^-24 T.

      one 16-bit plane    u |y| + c 2^-24 T        the stored value is the nearest 16-bit number to the fp32 result
      hi / lo pair        (3 u^2 + c 2^-24) T      the split of the output, two spare
      any fp16 plane      + 2^-25                  a plane value below 2^-14 is subnormal
    ReLU and the maximum are 1-Lipschitz and monotone and change nothing."""
    dt, pl = GEMM_PLANES[mode]
    u = GEMM_U[mode]
    floor = GEMM_F32_FLOOR_FACTOR * GN_F32_FLOOR_MEASURED * 2.0 ** -24 * T
    bound = u * y.abs() + floor if pl == 1 else 3.0 * u * u * T + floor
    if dt == torch.float16:
        bound = bound + 2.0 ** -25
    return bound


def scaled_pos_embed(C, seed=0, g_old=24):
    """pos_embed [1 + g_old^2, C] as fp32 values in fp64 (CPU): 2^((7 p mod 13) - 6) 2^((5 c mod 7) - 3) N(0, 1), p the row --
    the family of scaled_head_operands: every source pixel and every channel has a scale of its own."""
    g = torch.Generator().manual_seed(6000 + seed)
    n = 1 + g_old * g_old
    x = torch.randn(n, C, generator=g, dtype=torch.float64) * torch.exp2(_row_exp(n)).view(n, 1) * torch.exp2(_col_exp(C))
    return x.float().double()


def pos_axis64(g_old, g):
    """(i0, i1, l0, l1) of one axis of the half-pixel (align_corners=False) resize g_old -> g: the source coordinate is the
    exact rational s = max(((2 dst + 1) g_old - g) / (2 g), 0) (integers up to the one division), i0 = floor(s)."""
    dst = torch.arange(g, dtype=torch.float64)
    s = (((2.0 * dst + 1.0) * g_old - g) / (2.0 * g)).clamp_min(0.0)
    i0 = s.floor().to(torch.int64).clamp_max(g_old - 1)
    i1 = i0 + (i0 < g_old - 1).to(torch.int64)
    l1 = s - i0.double()
    return i0, i1, 1.0 - l1, l1


def pos_resize_ref64(src, g_old, gh, gw):
    """fp64 (y, Sb, L) [1 + gh gw, C] of _resize_pos_embed of src [1 + g_old^2, C]: row 0 is the cls row (Sb = |y|, L = 0); the
    grid rows are the bilinear blend ly0 (lx0 a + lx1 b) + ly1 (lx0 c + lx1 d) at pos_axis64's coordinates, Sb the same blend
    of |values|, and L the largest |a| + |b| + |c| + |d| over the 3 x 3 source cells around the cell (y0, x0): the interpolant
    is continuous and piecewise linear, so a coordinate that is off by e, even into a neighbouring cell, moves the value by at
    most e L."""
    src = src.double()
    C = src.shape[1]
    G = src[1:].view(g_old, g_old, C)
    y0, y1, ly0, ly1 = pos_axis64(g_old, gh)
    x0, x1, lx0, lx1 = pos_axis64(g_old, gw)
    ly0, ly1 = ly0.view(-1, 1, 1), ly1.view(-1, 1, 1)
    lx0, lx1 = lx0.view(1, -1, 1), lx1.view(1, -1, 1)
    a, b, c, d = G[y0][:, x0], G[y0][:, x1], G[y1][:, x0], G[y1][:, x1]
    y = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)
    Sb = ly0 * (lx0 * a.abs() + lx1 * b.abs()) + ly1 * (lx0 * c.abs() + lx1 * d.abs())
    nxt = torch.arange(g_old).add(1).clamp_max(g_old - 1)
    A = G.abs()
    cell = A + A[:, nxt] + A[nxt] + A[nxt][:, nxt]                                     # corner sum of the cell at (y, x)
    cp = torch.nn.functional.pad(cell, [0, 0, 1, 1, 1, 1], value=0.0)
    Lc = None
    for dy in range(3):
        for dx in range(3):
            s = cp[dy:dy + g_old, dx:dx + g_old]
            Lc = s if Lc is None else torch.maximum(Lc, s)
    L = Lc[y0][:, x0]
    z = torch.zeros(1, C, dtype=torch.float64)
    return (torch.cat([src[:1], y.reshape(-1, C)]), torch.cat([src[:1].abs(), Sb.reshape(-1, C)]), torch.cat([z, L.reshape(-1, C)]))


def pos_elem_bound(Sb, L):
    """Elementwise bar on |got - y| of the position-embedding resize: c 2^-24 Sb + e_s L with c = GEMM_F32_FLOOR_FACTOR x
    UP_F32_FLOOR_MEASURED = 18, the measured floor of the x2 up-sampling's blend (the same six products and three sums), and
    e_s = POS_COORD_ERR = 2^-18 the fp32 error of a source coordinate."""
    return GEMM_F32_FLOOR_FACTOR * UP_F32_FLOOR_MEASURED * 2.0 ** -24 * Sb + POS_COORD_ERR * L


# ------------------------------------------------------------------ conv + GroupNorm records, judged element by element
# The chain every bottleneck runs: the convolution's epilogue turns its fp32 accumulators into GroupNorm records (csrc/gemm_impl.h
# gn_records: (sum, sum of squares) per image, 32-row block and group), gn_affine_to_lds / gn_finalize_kernel (csrc/norm.hip)
# turn the records into the affines (a, d), and gn_apply_kernel or the C1_GN epilogue of csrc/conv1x1.hip applies them, with no
# shortcut, a plain one, or one behind a GroupNorm of its own.  The kernels that can be compared bit for bit share this code, so
# a mistake in it passes every such comparison; the helpers below give operands whose every (image, group) has a mean, a sigma
# and a ratio r = |mean| / sigma of its own, fp64 references of the records, the tables and the output, and the bar on every
# single one of them.  Everything is computed from conv_acc64 of the values the kernel reads.  Pure torch, any device.
# tests/test_gn_records_bound_host.py measures the constants and shows on a CPU which mistakes the bars reject;
# profiles/gn_records_elements.md has the figures.

GNREC_U = 2.0 ** -24
# Summation and cancellation constants of the statistics: the largest ratio of the fp32 model of
# tests/test_gn_records_bound_host.py -- gn_records' order (16 registers in sequence with fmaf for the squares, lane ^ 32, lane ^
# 1 .. cpg / 2), fp64 across the records in 8 slices, mean and rstd rounded to fp32 -- run on the fp64 accumulators rounded to
# fp32, to the fp64 reference, over GNREC_CASES and GNREC_APPLY_HOST x the four modes:
#   c_s   |s^ - s| / (u sum |v|)            of a record's sum
#   c_q   |q^ - q| / (u sum v^2)            of a record's sum of squares
#   c_a   |d rstd| / rstd / (u (1 + r^2))   one-pass variance: E[x^2] - mean^2 cancels 1 + r^2 to 1
#   c_m   |d mean| / (u (1 + r) sigma)
# Measured against the reference, never against a kernel; test_record_constants_are_what_the_bounds_use re-measures them.  The
# bars use GEMM_F32_FLOOR_FACTOR times these: the GPU's accumulators differ from the rounded fp64 ones within the GEMM bar, so
# every partial sum rounds differently.
GNREC_CS_MEASURED = 2.8
GNREC_CQ_MEASURED = 3.5
GNREC_CA_MEASURED = 2.5
GNREC_CM_MEASURED = 2.5
# (B, H, W, Cin, Cout, k, stride): every (Cin, Cout, k, stride) class of the ResNetV2 stages' convolutions, at B = 3 with
# 8 x 12 outputs (three records per image; M = 288: a block's waves straddle images) -- the stride-2 classes on 16 x 16 (two
# records) --, and B = 1 with 4 x 8 (one record).  3 x 3: TF-SAME padding, (1, 1) at stride 1 and (0, 1) at stride 2.
GNREC_CASES = ((3, 8, 12, 64, 64, 1, 1), (3, 8, 12, 256, 64, 1, 1), (3, 8, 12, 256, 128, 1, 1), (3, 8, 12, 512, 128, 1, 1),
               (3, 8, 12, 512, 256, 1, 1), (3, 8, 12, 1024, 256, 1, 1), (3, 8, 12, 64, 256, 1, 1), (3, 8, 12, 128, 512, 1, 1),
               (3, 8, 12, 256, 1024, 1, 1), (3, 16, 16, 256, 512, 1, 2), (3, 16, 16, 512, 1024, 1, 2),
               (3, 8, 12, 64, 64, 3, 1), (3, 8, 12, 128, 128, 3, 1), (3, 8, 12, 256, 256, 3, 1), (3, 16, 16, 128, 128, 3, 2),
               (3, 16, 16, 256, 256, 3, 2), (1, 4, 8, 64, 64, 1, 1), (1, 4, 8, 64, 256, 1, 1), (1, 4, 8, 256, 1024, 1, 1))
# (B, HW, C) of the apply pass alone on the CPU: HW = 2304 has 72 records, nine per slice of gn_affine_to_lds
GNREC_APPLY_HOST = ((2, 2304, 64), (1, 96, 1024), (2, 288, 64))


def conv_gn_geometry(case):
    """(pad, Ho, Wo) of a GNREC_CASES entry: TF-SAME, pad (1, 1) for 3 x 3 at stride 1, (0, 1) at stride 2, none for 1 x 1"""
    B, H, W, Cin, Cout, k, stride = case
    return (1 if (k == 3 and stride == 1) else 0), H // stride, W // stride


def conv_gn_operands(B, H, W, Cin, Cout, k, stride=1, seed=0):
    """X [B, H, W, Cin], Wt [Cout, k, k, Cin], gamma [Cout], beta [Cout], R [B, H / stride, W / stride, Cout] in fp64 (CPU),
    deterministic in `seed`, such that every (image, group) of conv(X, Wt) has a mean, a sigma and r = |mean| / sigma of its own:
      X[b, :, :, 0] = c_b = 2^((b mod 3) - 1) (1 - (b mod 3) / 4), a constant per image; the other channels 2^((b mod 3) - 1)
      N(0, 1) (for B <= 3 that is the scale 2^(b - 1) per image);
      Wt[n, :, :, 1:] = K^-1/2 2^((5 g) % 7 - 3) N(0, 1), g = n / cpg the group: sigma[b, g] ~ 2^((b mod 3) - 1) 2^((5 g) % 7 - 3);
      Wt[n, centre, centre, 0] = +-rho_g 2^((5 g) % 7 - 3) with rho_g = (0, 1.5, 8, 28)[g % 4] and the sign of (-1)^(g / 2), zero
      at every other tap: the centre tap lies inside the image wherever the output does, so zero padding does not move the
      mean at the border, which is c_b times that weight -- r[b, g] ~ rho_g (1, 3/4, 1/2)[b mod 3];
      gamma[c], beta[c] = 2^((5 c mod 7) - 3) N(0, 1): a scale per channel, either sign;
      R from the scaled_conv_operands family: a scale per pixel and per channel.
    |X| < 2 * 6, |conv| < 16 (28 + 6), |R| < 2^9 * 6, |gamma| 6 + |beta| + |R| < 60000: inside fp16.  r is measured by
    conv_gn_stats64 on the fp64 accumulators; assert_r_coverage holds every case to the coverage it needs."""
    g = torch.Generator().manual_seed(7000 + seed)
    cpg, K = Cout // 32, k * k * Cin
    bm = torch.arange(B) % 3
    sb = torch.exp2((bm - 1).double())
    X = torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64) * sb.view(B, 1, 1, 1)
    X[..., 0] = (sb * (1.0 - 0.25 * bm.double())).view(B, 1, 1)
    gi = torch.arange(32)
    sg = torch.exp2(((5 * gi) % 7 - 3).double())
    rho = torch.tensor([0.0, 1.5, 8.0, 28.0], dtype=torch.float64)[gi % 4] * torch.where((gi // 2) % 2 == 0, 1.0, -1.0).double()
    Wt = torch.randn(Cout, k, k, Cin, generator=g, dtype=torch.float64) * sg.repeat_interleave(cpg).view(-1, 1, 1, 1) * K ** -0.5
    Wt[..., 0] = 0.0
    Wt[:, k // 2, k // 2, 0] = (rho * sg).repeat_interleave(cpg)
    sc = torch.exp2(_col_exp(Cout))
    gamma = torch.randn(Cout, generator=g, dtype=torch.float64) * sc
    beta = torch.randn(Cout, generator=g, dtype=torch.float64) * sc
    R = scaled_conv_operands(B, H // stride, W // stride, 8, Cout, 1, seed)[3]
    return X, Wt, gamma, beta, R


def conv_gn_stats64(mode, acc, Sacc, eps=1e-5):
    """The fp64 references of the records and of the statistics, with their bars, from conv_acc64's (acc, Sacc) [B, Ho, Wo, C]
    of the values the kernel reads.  v = acc, S = Sacc, E = gemm_elem_bound(mode, v, S, 0, c_fp32=True) = F S (+ u16^2 S in the
    plane modes), the bar of one fp32 accumulator; u = 2^-24; sums run over the 32 rows x cpg channels of a record, mean_g over
    an (image, group); c_* = GEMM_F32_FLOOR_FACTOR x GNREC_C*_MEASURED.  Returns a dict of
      v [B, HW, C], E
      rec [B, HW / 32, 32, 2] = (s, q) = (sum v, sum v^2)
      rec_bar                 = (sum E + c_s u sum |v|,  2 sum |v| E + c_q u sum v^2)
      mean, var [B, 32] (biased, two-pass), sigma = sqrt(var + eps), r = |mean| / sigma
      mean_bar  = mean_g(E) + c_m u (1 + r) sigma
      rstd_rel  = (mean_g(|v| E) + |mean| mean_g(E)) / (var + eps) + c_a u (1 + r^2): the accumulators' error moves the second
                  moment by 2 mean_g(|v| E) and mean^2 by 2 |mean| mean_g(E), and d rstd / rstd = d var / (2 (var + eps))."""
    acc, Sacc = acc.double(), Sacc.double()
    B, C = acc.shape[0], acc.shape[-1]
    cpg = C // 32
    v, S = acc.reshape(B, -1, C), Sacc.reshape(B, -1, C)
    HW = v.shape[1]
    assert HW % 32 == 0
    E = gemm_elem_bound(mode, v, S, 0, c_fp32=True)
    u = GNREC_U
    cs, cq, ca, cm = (GEMM_F32_FLOOR_FACTOR * c for c in (GNREC_CS_MEASURED, GNREC_CQ_MEASURED, GNREC_CA_MEASURED, GNREC_CM_MEASURED))

    def blk(t):
        return t.reshape(B, HW // 32, 32, 32, cpg).sum((2, 4))

    s, q = blk(v), blk(v * v)
    s_bar = blk(E) + cs * u * blk(v.abs())
    q_bar = 2.0 * blk(v.abs() * E) + cq * u * q
    n = float(HW * cpg)
    mean = s.sum(1) / n
    var = ((v.reshape(B, HW, 32, cpg) - mean.view(B, 1, 32, 1)) ** 2).sum((1, 3)) / n
    sigma = torch.sqrt(var + eps)
    r = mean.abs() / sigma
    mE, mvE = blk(E).sum(1) / n, blk(v.abs() * E).sum(1) / n
    return dict(v=v, E=E, rec=torch.stack([s, q], -1), rec_bar=torch.stack([s_bar, q_bar], -1), mean=mean, var=var, sigma=sigma,
                r=r, mean_bar=mE + cm * u * (1.0 + r) * sigma, rstd_rel=(mvE + mean.abs() * mE) / (var + eps) + ca * u * (1.0 + r * r))


def assert_r_coverage(st):
    """the coverage a conv + GroupNorm case must have: a group that does not cancel (r <= 0.1), one that cancels 1 + r^2 >= 577
    to 1 (r >= 24), and none beyond what the operands are built for (r <= 40)"""
    r = st["r"]
    assert float(r.min()) <= 0.1 and float(r.max()) >= 24.0 and float(r.max()) <= 40.0, (float(r.min()), float(r.max()))


def gn_tables_ref64(st, gamma, beta):
    """The affines of a GroupNorm from conv_gn_stats64's statistics -- those of the fp64 ACCUMULATORS, which is what the
    records hold, not of the stored (rounded) map --: a = gamma rstd, d = beta - mean a [B, C] in fp64, with their bars
      a_bar = |a| (rstd_rel + u)                                 rstd_rel of conv_gn_stats64; u: a = rstd gamma is rounded
      d_bar = |a| mean_bar + |mean| a_bar + u (|mean| |a| + |beta|)   the last term: d = fma(-a, mean, beta) is rounded once
    Returns a dict of a, d, a_bar, d_bar, and per channel mean, |beta|, a_stat = |a| rstd_rel, m_stat = |a| mean_bar (what the
    statistics alone contribute to an output: gn_records_out_ref64)."""
    B = st["mean"].shape[0]
    C = gamma.numel()
    cpg = C // 32
    gamma, beta = gamma.double().view(1, C).to(st["mean"].device), beta.double().view(1, C).to(st["mean"].device)
    rep = lambda t: t.repeat_interleave(cpg, 1)
    mean, rstd, rel, mbar = rep(st["mean"]), rep(1.0 / st["sigma"]), rep(st["rstd_rel"]), rep(st["mean_bar"])
    a = gamma * rstd
    d = beta - mean * a
    a_bar = a.abs() * (rel + GNREC_U)
    d_bar = a.abs() * mbar + mean.abs() * a_bar + GNREC_U * (mean.abs() * a.abs() + beta.abs())
    return dict(a=a, d=d, a_bar=a_bar, d_bar=d_bar, mean=mean, beta=beta.abs().expand(B, C), a_stat=a.abs() * rel, m_stat=a.abs() * mbar)


def gn_records_out_ref64(mode, x, tab, R=None, rtab=None, relu=0):
    """fp64 (y, bound) [B, HW, C] of the apply pass: y = relu(x a + d [+ R | + R ra + rd]) of the STORED raw map x (hi + lo in
    the plane modes; gemm_elem_bound judges it against the accumulators) and shortcut R, with the tables of gn_tables_ref64.
      bound = gn_elem_bound(mode, y, T) + W
      T = |x| |a| + |mean| |a| + |beta|  [+ |R|  |  + |R| |ra| + |mean_r| |ra| + |beta_r|]      as gn_ref64, extended by the shortcut
      W = |x - mean| |a| rstd_rel + |a| mean_bar  [+ |R - mean_r| |ra| rstd_rel_r + |ra| mean_bar_r]
    W is what the statistics contribute, y = (x - mean) a + beta: |x - mean| |a| c_a u (1 + r^2) of the one-pass variance, and
    next to it the parts the table bars carry as well -- the accumulators' error in the moments and the error of the mean.
    The roundings of a, d and of the two fused multiply-adds are relative to terms of T and lie in gn_elem_bound's fp32 floor."""
    x = x.double()
    B, HW, C = x.shape
    t = {k: v.view(B, 1, C) for k, v in tab.items()}
    y = x * t["a"] + t["d"]
    T = x.abs() * t["a"].abs() + t["mean"].abs() * t["a"].abs() + t["beta"]
    Wd = (x - t["mean"]).abs() * t["a_stat"] + t["m_stat"]
    if R is not None:
        R = R.double().view(B, HW, C)
        if rtab is None:
            y, T = y + R, T + R.abs()
        else:
            s = {k: v.view(B, 1, C) for k, v in rtab.items()}
            y = y + R * s["a"] + s["d"]
            T = T + R.abs() * s["a"].abs() + s["mean"].abs() * s["a"].abs() + s["beta"]
            Wd = Wd + (R - s["mean"]).abs() * s["a_stat"] + s["m_stat"]
    y = torch.relu(y) if relu else y
    return y, gn_elem_bound(mode, y, T) + Wd


def gn_map_operands(B, HW, C, seed=0):
    """x [B, HW, C], gamma [C], beta [C], R [B, HW, C] in fp64 (CPU) for the apply pass alone: a raw map with the statistics
    conv_gn_operands gives a convolution's output -- x[b, p, c] = 2^((b mod 3) - 1) 2^((5 g) % 7 - 3) ((1, 3/4, 1/2)[b mod 3]
    rho_g + N(0, 1)), rho_g = +-(0, 1.5, 8, 28)[g % 4] -- and gamma, beta, R of the same families."""
    g = torch.Generator().manual_seed(7500 + seed)
    cpg = C // 32
    bm = torch.arange(B) % 3
    gi = torch.arange(32)
    sb = torch.exp2((bm - 1).double()).view(B, 1, 1, 1)
    sg = torch.exp2(((5 * gi) % 7 - 3).double()).view(1, 1, 32, 1)
    rho = (torch.tensor([0.0, 1.5, 8.0, 28.0], dtype=torch.float64)[gi % 4] * torch.where((gi // 2) % 2 == 0, 1.0, -1.0).double())
    z = torch.randn(B, HW, 32, cpg, generator=g, dtype=torch.float64).clamp(-5.0, 5.0)
    x = sb * sg * ((1.0 - 0.25 * bm.double()).view(B, 1, 1, 1) * rho.view(1, 1, 32, 1) + z)
    sc = torch.exp2(_col_exp(C))
    gamma = torch.randn(C, generator=g, dtype=torch.float64) * sc
    beta = torch.randn(C, generator=g, dtype=torch.float64) * sc
    R = scaled_gemm_operands(B * HW, C, 8, seed)[3].view(B, HW, C)
    return x.reshape(B, HW, C), gamma, beta, R


def records_of(x, cpg_groups=32):
    """fp32 records [B, HW / 32, 32, 2] of the values x [B, HW, C], computed in fp64 and rounded: what a perfect convolution
    epilogue would have left for the apply pass"""
    x = x.double()
    B, HW, C = x.shape
    t = x.reshape(B, HW // 32, 32, cpg_groups, C // cpg_groups)
    return torch.stack([t.sum((2, 4)), (t * t).sum((2, 4))], -1).float().contiguous()


def stats_of_records(rec, HW, cpg, eps=1e-5):
    """conv_gn_stats64's statistics dict from given fp32 records [B, nrec, 32, 2] taken as exact: the apply pass alone.  Its
    bars hold the summation terms only: fp64 across the records leaves the rounding of mean and rstd to fp32 (half a u each;
    mean_bar = u |mean|, rstd_rel = u) and the cancellation of E[x^2] - mean^2 in fp64, 2^-53 (1 + r^2), which is nothing."""
    rec = rec.double()
    n = float(HW * cpg)
    mean = rec[..., 0].sum(1) / n
    var = (rec[..., 1].sum(1) / n - mean * mean).clamp_min(0.0)
    sigma = torch.sqrt(var + eps)
    r = mean.abs() / sigma
    return dict(mean=mean, var=var, sigma=sigma, r=r, mean_bar=GNREC_U * mean.abs(), rstd_rel=GNREC_U + 0.0 * r)


# ------------------------------------------------------------------ outputs behind guards
SENTINEL =0xFFC1 - 0x10000  # int16 view of 0xFFC1: a NaN in bf16 and in fp16, which no kernel under test stores


class debug_flags:
    """with debug_flags(v): the launches inside run under dptx_debug_set_gemm_flags(v); 0 afterwards"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        assert load_library().dptx_debug_set_gemm_flags(self.value) == 0

    def __exit__(self, *exc):
        load_library().dptx_debug_set_gemm_flags(0)


class Target:
    """An output of n 16-bit elements (a hi / lo pair in the plane modes) pre-filled with a NaN, `guard` elements of the same
    NaN in front of it and behind it, and the inputs of one launch.  One plane: buffers of their own.  A pair: everything in
    one PlaneArena whose both planes are NaN wherever no input lies -- after the launch, whatever is not the output must
    hold the bits it held before."""

    def __init__(self, mode, n, guard, input_elems=0):
        self.mode, self.n, self.guard = mode, n, guard
        self.dt, self.pl = GEMM_PLANES[mode]
        if self.pl == 2:
            self.arena = PlaneArena(input_elems + n + 2 * guard + 4096, "cuda:0", self.dt)
            self.arena.buf.view(torch.int16).fill_(SENTINEL)
        else:
            self.arena = None

    def put(self, t):
        """an input: the values t rounded to the plane type, or split into the arena's planes"""
        return self.arena.put(t) if self.pl == 2 else t.float().to(self.dt).to("cuda:0").contiguous()

    def out(self):
        if self.pl == 2:
            self.arena.empty(self.guard)
            self.y = self.arena.empty(self.n)
            self.arena.empty(self.guard)
            self.before = self.arena.buf.clone()
        else:
            self.buf = torch.full((self.n + 2 * self.guard,), SENTINEL, device="cuda:0", dtype=torch.int16)
            self.y = self.buf[self.guard:self.guard + self.n].view(self.dt)
        return self.y

    def check(self):
        """nothing but the output was written"""
        torch.cuda.synchronize()
        if self.pl == 2:
            o = (self.y.data_ptr() - self.arena.buf.data_ptr()) // 2
            keep = torch.ones(self.arena.total, dtype=torch.bool, device="cuda:0")
            keep[o:o + self.n] = False
            a, b = self.arena.buf.view(torch.int16), self.before.view(torch.int16)
            assert torch.equal(a[:, keep], b[:, keep]), "written outside the output"
        else:
            g = self.guard
            assert bool((self.buf[:g] == SENTINEL).all()) and bool((self.buf[g + self.n:] == SENTINEL).all()), "written outside the output"

    def planes(self):
        """(hi, lo) planes of the output on the device, lo None for one plane, after check()"""
        self.check()
        return self.y, (self.arena.lo(self.y) if self.pl == 2 else None)

    def value(self):
        """fp64 value of the output (hi + lo) on the CPU, after check()"""
        self.check()
        return (self.arena.value(self.y) if self.pl == 2 else self.y.double()).cpu()

    def close(self):
        if self.arena is not None:
            self.arena.release()


def guarded_f32(n, guard):
    """(whole buffer, view of the n payload elements) of fp32 NaNs: `guard` of them in front of and behind the payload"""
    buf = torch.full((n + 2 * guard,), float("nan"), device="cuda:0")
    return buf, buf[guard:guard + n]


def f32_guards_intact(buf, n, guard):
    return bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all())


# ------------------------------------------------------------------ the UNet's head (last_bn + ReLU + last_conv2), element by element
# unet_gn_head_kernel (csrc/unet.hip) on a caller-supplied (mean, rstd) table: the operands of one case, the fp64 reference with
# its derived bound, and the kernel's arithmetic in fp32 on any device (the model tests/test_unet_bound_host.py mutates).
UNET_HEAD_OC = (1, 3, 4)
UNET_HEAD_HW = (1, 255, 257, 64 * 64)


def unet_head_operands(dtype, B, HW, OC, seed=0):
    """X [B, HW, 16] of nhwc_with_group_stats (groups = 8: every (image, pair of channels) has statistics of its own) rounded
    to the 16-bit type; stats [B, 8, 2] = (mean, rstd) of the stored values per (image, group) computed in fp64 (eps 1e-5) and
    rounded to fp32; gamma in [0.5, 1.5], beta in [-0.3, 0.3], w [OC, 16] ~ N(0, 1) 2^f_o / 4 and bias [OC] ~ N(0, 1) 2^f_o in
    fp32 (f_o = (5 o mod 7) - 3: every output channel a scale of its own).  CPU tensors."""
    X = nhwc_with_group_stats(B, HW, 16, groups=8, seed=500 + seed).to(TDT[dtype])
    xg = X.double().reshape(B, HW, 8, 2).transpose(1, 2).reshape(B, 8, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    stats = torch.stack([mean, 1.0 / torch.sqrt(var + 1e-5)], -1).float().contiguous()
    g = torch.Generator().manual_seed(600 + seed)
    gamma = (0.5 + torch.rand(16, generator=g)).float()
    beta = (0.6 * torch.rand(16, generator=g) - 0.3).float()
    so = torch.exp2(_col_exp(OC)).float()
    w = (torch.randn(OC, 16, generator=g) * so[:, None] * 0.25).float().contiguous()
    bias = (torch.randn(OC, generator=g) * so).float()
    return X, stats, gamma, beta, w, bias


def unet_head_ref64(X, stats, gamma, beta, w, bias):
    """(y, bound) in fp64, y [B, OC, HW]: y_o = bias_o + sum_j w_oj relu(x_j a_j + c_j) with a_j = rstd gamma_j and
    c_j = beta_j - mean a_j, of the fp32 table values as given (the kernel reads those, not the statistics of X).

    Bound, u = 2^-24, to first order in u.  The kernel rounds a_j once (a product), c_j once (one fused multiply-add of the
    ROUNDED a_j: its error is u |mean a_j| from a_j plus u |c_j| of its own), and the pre-activation once (one fused
    multiply-add: u |x_j a_j| from a_j, the error of c_j, and u |x_j a_j + c_j| <= u (|x_j a_j| + |c_j|) of its own):
      |f^_j - f_j| <= u T_j,  T_j = 2 |x_j a_j| + 2 |c_j| + |mean a_j|      (ReLU is 1-Lipschitz and changes nothing).
    The 16-term product is a chain of 16 fused multiply-adds that starts at the bias: every term passes through at most 16
    roundings, (1 + u)^16 - 1 < 17 u.  So |err| <= u (17 (|bias| + sum_j |w_j| f_j) + sum_j |w_j| T_j).  No measured constant."""
    u = 2.0 ** -24
    B, HW, _ = X.shape
    x = X.double()
    mean = stats[..., 0].double().repeat_interleave(2, 1).view(B, 1, 16)
    rstd = stats[..., 1].double().repeat_interleave(2, 1).view(B, 1, 16)
    a = rstd * gamma.double()
    c = beta.double() - mean * a
    f = torch.relu(x * a + c)                                              # [B, HW, 16]
    T = 2.0 * (x * a).abs() + 2.0 * c.abs() + (mean * a).abs()
    wd, bd = w.double(), bias.double()
    y = f @ wd.t() + bd
    bound = u * (17.0 * (bd.abs() + f @ wd.abs().t()) + T @ wd.abs().t())
    return y.transpose(1, 2).contiguous(), bound.transpose(1, 2).contiguous()


def _fma32(a, b, c):
    """fl32(a b + c) of fp32 tensors: the product of two fp32 numbers is exact in fp64, the sum is rounded to fp64 and then to
    fp32 (a double rounding differs from the fused result in about one element in 2^29, by one ulp)"""
    return (a.double() * b.double() + c.double()).float()


def unet_head_model32(X, stats, gamma, beta, w, bias, mutant=None, dtype=None):
    """The kernel's arithmetic in fp32, in its order -> y [B, OC, HW] fp32.  mutant: 'round16' (the normalised values rounded
    to the 16-bit type `dtype` before the 1x1), 'beta_shift' (beta of channel j + 1 used for channel j), 'late_relu' (the
    ReLU behind the 1x1 instead of in front of it)."""
    B, HW, _ = X.shape
    x = X.float()
    mean = stats[..., 0].repeat_interleave(2, 1).view(B, 1, 16)
    rstd = stats[..., 1].repeat_interleave(2, 1).view(B, 1, 16)
    a = rstd * gamma.float()
    be = beta.float().roll(-1) if mutant == "beta_shift" else beta.float()
    c = _fma32(-mean, a, be.view(1, 1, 16).expand(B, 1, 16))
    f = _fma32(x, a.expand(B, HW, 16), c.expand(B, HW, 16))
    if mutant != "late_relu":
        f = torch.relu(f)
    if mutant == "round16":
        f = f.to(TDT[dtype]).float()
    s = bias.float().view(1, 1, -1).expand(B, HW, -1)
    for j in range(16):
        s = _fma32(f[..., j:j + 1], w.float()[:, j].view(1, 1, -1), s)
    if mutant == "late_relu":
        s = torch.relu(s)
    return s.transpose(1, 2).contiguous()
