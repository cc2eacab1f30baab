"""Guided upsampling (include/dptx.h, "Guided upsampling") restated in torch, with no dependency on the library: the same taps in
the same (qy, qx) order, the same e - e_min form, every operation rounded on its own in `dtype` (torch.float32: the definition
itself; torch.float64: the yardstick the device and the fp32 restatement are measured against).

What both dtypes share, because the definition fixes it in fp32: the source coordinates sy, sx (ATen's align_corners=False
coordinate with scale = in / out in fp32) and with them floor(sy), floor(sx) -- the tap set must not depend on the yardstick's
precision -- and ks = 1 / (2 sigma_space^2), kr = 1 / (2 sigma_range^2), computed in double and rounded once to fp32."""
import numpy as np
import torch


def constants(sigma_space, sigma_range):
    """-> (ks, kr) as the host computes them: double arithmetic on the fp32 parameters, one rounding to fp32."""
    ss, sr = float(np.float32(sigma_space)), float(np.float32(sigma_range))
    return float(np.float32(1.0 / (2.0 * ss * ss))), float(np.float32(1.0 / (2.0 * sr * sr)))


def _coords(n_in, n_out):
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    s = scale * (torch.arange(n_out, dtype=torch.float32) + 0.5) - 0.5
    return s, torch.floor(s).long()


def guide_hi(pixels_u8, dtype):
    """uint8 [H,W], [H,W,1] or [H,W,3] -> [3,H,W]: u8 / 255 in `dtype`, a grey image's channel three times."""
    g = torch.as_tensor(np.asarray(pixels_u8))
    if g.ndim == 2:
        g = g[:, :, None]
    g = g.permute(2, 0, 1).to(dtype) / 255
    return g.expand(3, -1, -1) if g.shape[0] == 1 else g


def guided_values(S, G_lo, pixels_u8, radius=2, sigma_space=1.0, sigma_range=0.1, dtype=torch.float64):
    """Steps 1-5: S [C,h,w], G_lo [3,h,w], pixels_u8 [H,W(,1|3)] uint8 -> v [C,H,W] in `dtype`."""
    C, h, w = S.shape
    gh = guide_hi(pixels_u8, dtype)
    H, W = gh.shape[1:]
    S, G_lo = S.to(dtype), G_lo.to(dtype)
    ks, kr = (torch.tensor(k, dtype=dtype) for k in constants(sigma_space, sigma_range))
    (sy, by), (sx, bx) = _coords(h, H), _coords(w, W)
    R = int(radius)
    taps, exps = [], []
    for j in range(2 * R):
        qy = by - R + 1 + j
        oky, qyc = (qy >= 0) & (qy < h), qy.clamp(0, h - 1)
        dy = qy.to(dtype) - sy.to(dtype)
        for i in range(2 * R):
            qx = bx - R + 1 + i
            okx, qxc = (qx >= 0) & (qx < w), qx.clamp(0, w - 1)
            dx = qx.to(dtype) - sx.to(dtype)
            d2 = (dy * dy)[:, None] + (dx * dx)[None, :]
            diff = gh - G_lo[:, qyc][:, :, qxc]
            rr = diff[0] * diff[0]
            rr = rr + diff[1] * diff[1]
            rr = rr + diff[2] * diff[2]
            e = ks * d2 + kr * rr
            valid = oky[:, None] & okx[None, :]
            exps.append(torch.where(valid, e, torch.full_like(e, float("inf"))))
            taps.append((qyc, qxc, valid))
    emin = torch.stack(exps).amin(0)
    den = torch.zeros(H, W, dtype=dtype)
    acc = torch.zeros(C, H, W, dtype=dtype)
    for e, (qyc, qxc, valid) in zip(exps, taps):
        wgt = torch.where(valid, torch.exp(-(e - emin)), torch.zeros_like(e))   # a skipped tap adds nothing
        den = den + wgt
        acc = acc + wgt[None] * S[:, qyc][:, :, qxc]
    return acc / den


def finish(v, mode, renormalize=False):
    """Step 6 in v's dtype: 'normal_f32' / 'normal_u8' [3,H,W] -> [3,H,W] float / [H,W,3] uint8; 'depth_f32' [1,H,W] -> [H,W]."""
    if mode.startswith("normal"):
        if renormalize:
            n = 2 * v - 1
            ss = n[0] * n[0]
            ss = ss + n[1] * n[1]
            ss = ss + n[2] * n[2]
            v = (n / torch.sqrt(ss).clamp_min(1e-12) + 1) / 2
        v = v.clamp(0, 1)
        return v if mode == "normal_f32" else (v * 255).to(torch.uint8).permute(1, 2, 0).contiguous()
    assert mode == "depth_f32"
    return 1 - v[0].clamp(0, 1)


def guided_restatement(S, G_lo, pixels_u8, mode, renormalize=False, radius=2, sigma_space=1.0, sigma_range=0.1, dtype=torch.float64):
    return finish(guided_values(S, G_lo, pixels_u8, radius, sigma_space, sigma_range, dtype), mode, renormalize)


def planted_case(h=96, w=128, factor=8, noise=0.02, seed=0):
    """A two-region piecewise-constant truth [1,h,w] at full resolution, its antialiased (box-averaged) `factor`-times smaller copy,
    a noisy two-colour uint8 guide of the full resolution and the guide's box-averaged low-resolution copy.
    -> (truth [1,h,w], S [1,h/f,w/f], G_lo [3,h/f,w/f], pixels [h,w,3] uint8), fp64 / uint8."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    region = (xx + 0.35 * yy + 6 * torch.sin(yy / 9)) > 0.55 * w          # a slanted, wavy boundary
    truth = torch.where(region, 0.8, 0.2)[None]
    colours = torch.tensor([[0.75, 0.35, 0.2], [0.15, 0.45, 0.7]], dtype=torch.float64)
    rgb = torch.where(region[None], colours[0][:, None, None], colours[1][:, None, None])
    rgb = (rgb + noise * torch.randn(3, h, w, generator=g, dtype=torch.float64)).clamp(0, 1)
    pixels = (rgb * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
    pool = torch.nn.AvgPool2d(factor)
    S = pool(truth[None])[0]
    G_lo = pool((pixels.permute(2, 0, 1).double() / 255)[None])[0]
    return truth, S, G_lo, pixels.numpy()
