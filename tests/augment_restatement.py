"""The definitions of include/dptx.h, "Training augmentations", in torch ops on the CPU, in the precision `dtype`: run in fp32 they
are the definition up to the order of roundings (mul + add where the kernel fuses), run in fp64 they are the reference the GPU
tests and the host build are judged against.  The tap tables, the factors and the resize coordinates are fp32 values in both
precisions: they are the kernel's inputs, not part of its arithmetic."""
import numpy as np
import torch
import torch.nn.functional as F


def _per_sample(v, B, dtype):
    return torch.as_tensor(v, dtype=torch.float32).reshape(-1).expand(B).to(dtype).view(B, 1, 1, 1)


def sharpness(x, factor, dtype=torch.float32):
    """x [B,C,H,W]; factor: a number or [B]"""
    x = x.to(dtype)
    B, _, H, W = x.shape
    d = x.clone()
    if H >= 3 and W >= 3:
        a, b = torch.tensor(1.0 / 13.0, dtype=torch.float32).to(dtype), torch.tensor(5.0 / 13.0, dtype=torch.float32).to(dtype)
        acc = torch.zeros_like(x[:, :, 1:-1, 1:-1])
        for r in range(3):
            for q in range(3):
                acc = acc + (b if r == 1 and q == 1 else a) * x[:, :, r:H - 2 + r, q:W - 2 + q]
        d[:, :, 1:-1, 1:-1] = acc
    f = _per_sample(factor, B, dtype)
    return torch.where(f == 1, x, d + (x - d) * f)


def motion_blur(x, taps, dtype=torch.float32):
    """x [B,C,H,W]; taps [B,k,k] fp32: correlation with zero padding"""
    x = x.to(dtype)
    B, _, H, W = x.shape
    k = taps.shape[-1]
    t = taps.to(torch.float32).to(dtype)
    xp = F.pad(x, (k // 2,) * 4)
    acc = torch.zeros_like(x)
    for r in range(k):
        for q in range(k):
            acc = acc + t[:, r, q].view(B, 1, 1, 1) * xp[:, :, r:r + H, q:q + W]
    return acc


def gaussian_blur(x, gy, gx, dtype=torch.float32):
    """x [B,C,H,W]; gy [B,ky], gx [B,kx] fp32: weights gy[i] * gx[j] (one fp32 product), reflect border"""
    x = x.to(dtype)
    B, _, H, W = x.shape
    ky, kx = gy.shape[-1], gx.shape[-1]
    w = (gy.to(torch.float32).view(B, ky, 1) * gx.to(torch.float32).view(B, 1, kx)).to(dtype)
    xp = F.pad(x, (kx // 2, kx // 2, ky // 2, ky // 2), mode="reflect") if max(ky, kx) > 1 else x
    acc = torch.zeros_like(x)
    for i in range(ky):
        for j in range(kx):
            acc = acc + w[:, i, j].view(B, 1, 1, 1) * xp[:, :, i:i + H, j:j + W]
    return acc


def chain(x, sharp=None, motion=None, gauss=None, dtype=torch.float32):
    """sharp: factor(s); motion: taps [B,k,k]; gauss: (gy [B,ky], gx [B,kx]); None skips the stage"""
    y = x.to(dtype)
    if sharp is not None:
        y = sharpness(y, sharp, dtype)
    if motion is not None:
        y = motion_blur(y, motion, dtype)
    if gauss is not None:
        y = gaussian_blur(y, gauss[0], gauss[1], dtype)
    return y


def crop(t, y0, x0, h, w):
    return t[:, :, y0:y0 + h, x0:x0 + w].clone()


def nearest_index(n_in, n_out):
    scale = np.float32(n_in) / np.float32(n_out)
    i = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return torch.from_numpy(np.minimum(i, n_in - 1))


def resize_nearest(t, h, w):
    return t[:, :, nearest_index(t.shape[2], h)][:, :, :, nearest_index(t.shape[3], w)].clone()


def linear_axis(n_in, n_out, fused=False):
    """(i0, i1, l0, l1): indices int64, weights fp32 -- ATen's align_corners=False coordinates in fp32.  fused: the coordinate
    is one fused multiply-subtract, fma(scale, dst + 0.5, -0.5) (the product of two fp32 numbers and its difference to 0.5 are
    exact in fp64, so the fp64 expression rounded once is that fma)."""
    dst = np.arange(n_out, dtype=np.float32)
    if n_in == n_out:
        i = torch.arange(n_out)
        return i, i, torch.ones(n_out), torch.zeros(n_out)
    scale = np.float32(n_in) / np.float32(n_out)
    if fused:
        real = (np.float64(scale) * (dst.astype(np.float64) + 0.5) - 0.5).astype(np.float32)
    else:
        real = scale * (dst + np.float32(0.5)) - np.float32(0.5)
    real = np.maximum(real, np.float32(0))
    i0 = np.minimum(np.floor(real).astype(np.int64), n_in - 1)
    l1 = np.clip(real - i0.astype(np.float32), np.float32(0), np.float32(1)).astype(np.float32)
    i1 = i0 + (i0 < n_in - 1)
    l0 = np.float32(1) - l1
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l0), torch.from_numpy(l1)


def resize_bilinear(t, h, w, dtype=torch.float32):
    t = t.to(dtype)
    y0, y1, ly0, ly1 = linear_axis(t.shape[2], h)
    x0, x1, lx0, lx1 = linear_axis(t.shape[3], w)
    ly0, ly1 = ly0.to(dtype).view(-1, 1), ly1.to(dtype).view(-1, 1)
    lx0, lx1 = lx0.to(dtype), lx1.to(dtype)
    r0, r1 = t[:, :, y0], t[:, :, y1]
    t0 = lx0 * r0[..., x0] + lx1 * r0[..., x1]
    t1 = lx0 * r1[..., x0] + lx1 * r1[..., x1]
    return ly0 * t0 + ly1 * t1


def resize_bilinear_aten_cpu(t, h, w):
    """What CPU ATen's vectorised kernel computes for F.interpolate(t, (h, w), mode='bilinear') of a small fp32 tensor -- the
    arithmetic of the reference's recorded outputs (tests/golden/augment_resize_*.npz), recovered from ATen's results: delta
    images give its weights, zeroed rows and the 24 orders of a four-term sum its order.  NOT the kernel's definition
    (resize_bilinear): the same coordinates and weights up to fusing, another order of roundings.
      coordinate   fma(scale, dst + 0.5, -0.5), then ATen's guard; l1 = coordinate - i0, l0 = 1 - l1
      weights      w00 = ly0 * lx0, w01 = ly0 * lx1, w10 = ly1 * lx0, w11 = ly1 * lx1, one fp32 product each
      value        acc = w01 * b;  acc = fma(w00, a, acc);  acc = fma(w10, c, acc);  acc = fma(w11, d, acc)
                   with a, b the row i0's two pixels and c, d the row i1's
    An fma of fp32 numbers is formed in fp64: the product is exact there, and the sum is rounded to fp64 and then to fp32.
    Larger tensors (512 x 512 -> 384 x 448) go through another ATen kernel, fma(l0, a, l1 * b) per axis; not modelled here."""
    t = t.float()
    y0, y1, ly0, ly1 = linear_axis(t.shape[2], h, fused=True)
    x0, x1, lx0, lx1 = linear_axis(t.shape[3], w, fused=True)
    ly0, ly1 = ly0.view(-1, 1), ly1.view(-1, 1)
    r0, r1 = t[:, :, y0], t[:, :, y1]
    a, b, c, d = r0[..., x0], r0[..., x1], r1[..., x0], r1[..., x1]
    acc = (ly0 * lx1) * b
    for wt, v in ((ly0 * lx0, a), (ly1 * lx0, c), (ly1 * lx1, d)):
        acc = (wt.double() * v.double() + acc.double()).float()
    return acc
