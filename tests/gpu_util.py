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
