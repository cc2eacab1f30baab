"""The definition of dptx_eval_depth_aligned (include/dptx.h) in torch, on any device: fp32 where the kernel is fp32 (the aligned
value, every step rounded on its own), fp64 where it is fp64 (the sums of the fit, every metric).  It is the statement of fields
8-14 (abs_rel, sq_rel, rmse, rmse_log, delta1..3), which the reference does not have; fields 0-7 restate
paper_code/evaluation_metrics.py:61-79 and the fits restate losses/midas_loss.py:10-56.

    stats(pred, target, mask, dtype)     -> dict of [B] tensors: t_p, t_g, s_p, s_g, scale, shift, sums in `dtype`
    aligned(pred, align, st, clamp)      -> [B,1,H,W] fp32
    coeffs(align, st)                    -> [B,2] fp32: the reported (scale, shift)
    rows(al, target, mask, min_depth)    -> [B + 1, 15] fp64: rows 0..B-1 the images, row B the batch
    inputs(seed, B, H, W)                -> the test case of the suite: pred, target [B,1,H,W] fp32, mask [B,1,H,W] bool
"""
import numpy as np
import torch

FIELDS = ("num_valid", "eval_L1", "eval_mse", "log10_diff", "log10", "si_log", "rel_error", "irmse",
          "abs_rel", "sq_rel", "rmse", "rmse_log", "delta1", "delta2", "delta3")
THRESHOLDS = (1.25, 1.5625, 1.953125)
EPS = 1e-6


def smooth(rng, B, H, W, lo, hi, k=6):
    """[B,1,H,W] fp32 smooth random field in [lo, hi] (bilinear upsampling of a coarse grid)"""
    g = torch.from_numpy(rng.random((B, 1, k, k)).astype(np.float32))
    f = torch.nn.functional.interpolate(g, size=(H, W), mode="bilinear", align_corners=True)
    f = (f - f.amin((2, 3), keepdim=True)) / (f.amax((2, 3), keepdim=True) - f.amin((2, 3), keepdim=True))
    return (lo + (hi - lo) * f).float().contiguous()


def inputs(seed, B, H, W, noise=0.02, field=0.05, keep=0.8):
    """a smooth target in [0.1, 0.9]; the prediction is the target seen through (t - 0.2) / 1.7 plus a smooth +-field plus
    N(0, noise); 80 % of the pixels valid"""
    rng = np.random.default_rng(seed)
    t = smooth(rng, B, H, W, 0.1, 0.9)
    p = (t - 0.2) / 1.7
    if field:
        p = p + smooth(rng, B, H, W, -field, field)
    if noise:
        p = p + torch.from_numpy(rng.normal(0.0, noise, t.shape).astype(np.float32))
    m = torch.from_numpy(rng.random(t.shape) < keep)
    return p.float().contiguous(), t, m


def stats(pred, target, mask, dtype=torch.float64):
    """The per-image statistics of both fits with sums in `dtype`, every result rounded to fp32 (fp64: what the kernels
    compute; fp32: the reference's own run).  The medians are lower nanmedians of the valid values, 0 without one."""
    B = pred.shape[0]
    p, t = pred.reshape(B, -1).to(dtype), target.reshape(B, -1).to(dtype)
    m = mask.reshape(B, -1)
    mf = m.to(dtype)
    n = mf.sum(1)
    out = {}
    for name, x in (("p", p), ("g", t)):
        med = torch.where(m, x, torch.full_like(x, float("nan"))).nanmedian(1).values
        med = torch.where(torch.isnan(med), torch.zeros_like(med), med)
        out["t_" + name] = med.float()
        out["s_" + name] = ((x - med[:, None]).abs() * mf).sum(1).div(n + 1).float()
    a00, a01, b0, b1 = (mf * p * p).sum(1), (mf * p).sum(1), (mf * p * t).sum(1), (mf * t).sum(1)
    det = a00 * n - a01 * a01
    ok = det != 0
    out["scale"] = torch.where(ok, (n * b0 - a01 * b1) / (det + 1e-6), torch.zeros_like(det)).float()
    out["shift"] = torch.where(ok, (-a01 * b0 + a00 * b1) / (det + 1e-6), torch.zeros_like(det)).float()
    return out


def aligned(pred, align, st, clamp):
    """fp32, every step rounded on its own (torch evaluates each op separately: nothing is fused)"""
    p = pred.float()
    v = lambda k: st[k].float().to(p.device).view(-1, 1, 1, 1)
    if align == "lstsq":
        a = v("scale") * p
        a = a + v("shift")
    elif align == "median":
        pa = (p - v("t_p")) / (v("s_p") + np.float32(EPS))
        a = pa * (v("s_g") + np.float32(EPS))
        a = a + v("t_g")
    else:
        raise ValueError(align)
    return a.clamp(0, 1) if clamp else a


def coeffs(align, st):
    if align == "lstsq":
        return torch.stack([st["scale"].float(), st["shift"].float()], 1)
    sc = (st["s_g"].float() + np.float32(EPS)) / (st["s_p"].float() + np.float32(EPS))
    return torch.stack([sc, st["t_g"].float() - sc * st["t_p"].float()], 1)


def _row(a, t, m, min_depth):
    """one row from flat fp64 aligned prediction, target and bool mask"""
    nan = float("nan")
    n = float(m.sum())
    if n < 1:
        return [0.0] + [nan] * (len(FIELDS) - 1)
    mf = m.double()
    inv = m.numel() / n
    diff = (a - t).abs() * mf
    dlog = ((torch.log(1 + 64 * a) - torch.log(1 + 64 * t)) * mf).abs()
    row = [n, float(diff.mean() * inv * 100), float((diff ** 2).mean() * inv * 100), float((torch.log(1 + 64 * diff) * mf).mean() * inv),
           float(dlog.mean() * inv), float((dlog ** 2).sum() / n - dlog.sum() ** 2 / n ** 2), float(((diff / t) * mf).mean() * inv),
           float((((1 / (1 + 64 * a) - 1 / (1 + 64 * t)) ** 2) * mf).mean() * inv)]
    ae, te = a[m].clamp(min=min_depth), t[m].clamp(min=min_depth)   # the valid pixels only; a NaN stays a NaN
    d = ae - te
    ratio = torch.maximum(ae / te, te / ae)
    row += [float((d.abs() / te).mean()), float((d * d / te).mean()), float((d * d).mean().sqrt()),
            float(((torch.log(ae) - torch.log(te)) ** 2).mean().sqrt())]
    row += [float((ratio < th).sum()) / n for th in THRESHOLDS]   # a NaN compares false
    return row


def rows(al, target, mask, min_depth=1e-3):
    B = al.shape[0]
    a, t, m = al.double().reshape(B, -1).cpu(), target.double().reshape(B, -1).cpu(), mask.reshape(B, -1).cpu()
    md = float(np.float32(min_depth))   # the C ABI takes a float
    out = [_row(a[i], t[i], m[i], md) for i in range(B)]
    out.append(_row(a.reshape(-1), t.reshape(-1), m.reshape(-1), md))
    return torch.tensor(out, dtype=torch.float64)


def ratio_margin(al, target, mask, min_depth=1e-3):
    """the smallest relative distance of a valid pixel's ratio max(a_e / t_e, t_e / a_e) to a delta threshold"""
    md = float(np.float32(min_depth))
    ae, te = al.double()[mask].clamp(min=md), target.double()[mask].clamp(min=md)
    r = torch.maximum(ae / te, te / ae)
    return min(float(((r - th).abs() / th).min()) for th in THRESHOLDS) if r.numel() else float("inf")
