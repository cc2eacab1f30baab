"""Torch restatement of the reference's MiDaS loss (omnidata_tools/torch/losses/midas_loss.py) and of its gradient with
respect to the prediction, the yardstick of tests/test_midas_host.py and tests/test_gpu_midas.py.

`forward` follows the numerics policy of csrc/midas_loss.hip: the per-pixel values the reference keeps as tensors
(1/(x + 1e-6), t, s, a, g, scale, shift, r, d) in `dt`, each step rounded on its own (fp32 when compared with the
kernels), every sum and the 2x2 solve in fp64.  It also gives the gradient in closed form (fp64).  `plain_loss` is the
loss written directly with differentiable torch ops, for autograd.  No reference code is imported.
"""
from __future__ import annotations

import numpy as np
import torch

EPS = 1e-6
SSI, GRAD, ALIGN, INVERSE = 1, 2, 4, 8
ALL = SSI | GRAD | ALIGN | INVERSE


def medians(x: torch.Tensor, valid: torch.Tensor):
    """Lower nanmedian of the valid values of every row of x [B, N] (0 without a non-NaN one) and the argmedian: the lowest
    index of a valid value equal to it (-1 without)."""
    B = x.shape[0]
    t = x.masked_fill(~valid, float("nan")).nanmedian(-1).values
    has = ~torch.isnan(t)
    t = torch.where(has, t, torch.zeros_like(t))
    hit = valid & (x == t[:, None]) & has[:, None]
    idx = torch.where(hit.any(1), hit.to(torch.int64).argmax(1), torch.full((B,), -1, dtype=torch.int64))
    return t, idx


def forward(pred, target, mask, terms=ALL, scales=4, image_based=True, alpha=0.1, dt=torch.float32, grad_losses=None,
            kink_rel=1e-5):
    """pred, target [B,H,W] float, mask [B,H,W] bool (CPU) -> dict: losses (total, ssi, reg) in fp64 before the final
    rounding, per-image t_p, t_g, s_p, s_g, n, scale, shift, argmedian, the aligned tensors, the pixels with a kink argument
    below kink_rel of its operands (ssi_kink: a - g; reg_kink: a pair difference of d), and with
    grad_losses = (g_total, g_ssi, g_reg) the gradient with respect to pred (fp64).  The reference multiplies by alpha in
    fp32: alpha is rounded to fp32 here too."""
    p, g, m = pred.to(dt), target.to(dt), mask.bool()
    B, H, W = p.shape
    e = torch.tensor(EPS, dtype=dt)
    alpha = float(np.float32(alpha))
    pf, gf, mf = p.reshape(B, -1), g.reshape(B, -1), m.reshape(B, -1)
    n = mf.sum(1).double()
    N = n.sum()
    z = torch.zeros((), dtype=torch.float64)
    out = dict(n=n, ssi=z, reg=z)
    grad = torch.zeros(B, H * W, dtype=torch.float64)
    if grad_losses is not None:
        g0, g1, g2 = (float(v) for v in grad_losses)
        w_ssi = g0 + g1
        w_reg = (alpha if terms & SSI else 1.0) * g0 + g2
    if terms & SSI:
        tp, med = medians(pf, mf)
        tg, _ = medians(gf, mf)
        up, ug = pf - tp[:, None], gf - tg[:, None]
        sp = (torch.where(mf, up.abs().double(), z).sum(1) / (n + 1)).to(dt)
        sg = (torch.where(mf, ug.abs().double(), z).sum(1) / (n + 1)).to(dt)
        Dp, Dg = sp + e, sg + e
        a, ga = up / Dp[:, None], ug / Dg[:, None]
        diff = a - ga
        out["ssi"] = torch.where(mf, diff.abs().double(), z).sum() / N
        out.update(t_p=tp, t_g=tg, s_p=sp, s_g=sg, argmedian=med, pred_aligned=a.reshape(B, H, W),
                   target_aligned=ga.reshape(B, H, W))
        # SSI kink: |a - g| small against |a|, |g| (a = g = 0 exactly is no kink: both sides compute 0)
        size = torch.maximum(a.abs(), ga.abs()).double()
        out["ssi_kink"] = (mf & (diff.abs().double() <= kink_rel * size) & (size > 0)).reshape(B, H, W)
        if grad_losses is not None and N > 0:
            sd, su = torch.sign(diff.double()), torch.sign(up.double())
            E = torch.where(mf, sd, z).sum(1)
            EU = torch.where(mf, sd * up.double(), z).sum(1)
            SU = torch.where(mf, su, z).sum(1)
            D = Dp.double()
            kd = 1.0 / (N * D)
            ks = EU / (N * D * D * (n + 1))
            kmed = -E * kd + SU * ks
            gs = torch.where(mf, kd[:, None] * sd - ks[:, None] * su, z)
            for b in range(B):
                if med[b] >= 0:
                    gs[b, med[b]] += kmed[b]
            grad += w_ssi * gs
            out["kd"] = kd
    if terms & GRAD:
        x = torch.reciprocal(p + e) if terms & INVERSE else p
        y = torch.reciprocal(g + e) if terms & INVERSE else g
        md, xd, yd = m.double(), x.double(), y.double()
        ok = torch.zeros(B, dtype=torch.bool)
        if terms & ALIGN:
            a00, a01, a11 = (md * xd * xd).sum((1, 2)), (md * xd).sum((1, 2)), n
            b0, b1 = (md * xd * yd).sum((1, 2)), (md * yd).sum((1, 2))
            det = a00 * a11 - a01 * a01
            ok = det != 0
            Q = det + 1e-6
            X0, X1 = (a11 * b0 - a01 * b1) / Q, (-a01 * b0 + a00 * b1) / Q
            scale = torch.where(ok, X0, z).to(dt)
            shift = torch.where(ok, X1, z).to(dt)
            r = scale[:, None, None] * x + shift[:, None, None]
            out.update(scale=scale, shift=shift, det_ok=ok)
        else:
            r = x
        d = m.to(dt) * (r - y)
        Ls, Ms = [], []
        G = torch.zeros(B, H, W, dtype=torch.float64)
        kink = torch.zeros(B, H, W, dtype=torch.bool)
        for k in range(scales):
            s = 2 ** k
            ds, ms = d[:, ::s, ::s], m[:, ::s, ::s]
            mt = ms.to(dt)
            gx, gy = ds[:, :, 1:] - ds[:, :, :-1], ds[:, 1:, :] - ds[:, :-1, :]
            mx, my = mt[:, :, 1:] * mt[:, :, :-1], mt[:, 1:, :] * mt[:, :-1, :]
            Ls.append((mx * gx.abs()).double().sum((1, 2)) + (my * gy.abs()).double().sum((1, 2)))
            Ms.append(ms.sum((1, 2)).double())
            # reg kink: a pair difference that is non-zero but small against the pair's values
            ad = ds.abs().double()
            kx = (mx > 0) & (gx != 0) & (gx.abs().double() <= kink_rel * torch.maximum(ad[:, :, 1:], ad[:, :, :-1]))
            ky = (my > 0) & (gy != 0) & (gy.abs().double() <= kink_rel * torch.maximum(ad[:, 1:, :], ad[:, :-1, :]))
            kk = torch.zeros(ds.shape, dtype=torch.bool)
            kk[:, :, 1:] |= kx
            kk[:, :, :-1] |= kx
            kk[:, 1:, :] |= ky
            kk[:, :-1, :] |= ky
            kink[:, ::s, ::s] |= kk
            if grad_losses is not None:
                if image_based:
                    wk = torch.where(Ms[k] > 0, 1.0 / (B * Ms[k].clamp_min(1)), z)
                else:
                    wk = (1.0 / Ms[k].sum() if Ms[k].sum() > 0 else z).expand(B)
                sx, sy = torch.sign(gx.double()) * mx.double(), torch.sign(gy.double()) * my.double()
                Gs = torch.zeros(ds.shape, dtype=torch.float64)
                Gs[:, :, 1:] += sx
                Gs[:, :, :-1] -= sx
                Gs[:, 1:, :] += sy
                Gs[:, :-1, :] -= sy
                G[:, ::s, ::s] += wk[:, None, None] * Gs
        L, M = torch.stack(Ls), torch.stack(Ms)      # [scales, B]
        if image_based:
            reg = (torch.where(M != 0, L / M.clamp_min(1), L).sum(1) / B).sum()
        else:
            reg = z
            for k in range(scales):
                reg = reg + (L[k].sum() / M[k].sum() if M[k].sum() != 0 else z)
        out.update(reg=reg, L=L, M=M, reg_kink=kink, d=d)
        if grad_losses is not None:
            dx = G
            if terms & ALIGN:
                S, T = (G * xd).sum((1, 2)), G.sum((1, 2))
                c00 = torch.where(ok, S * (-X0 * a11 / Q) + T * (b1 / Q - X1 * a11 / Q), z)
                c01 = torch.where(ok, S * ((2.0 * a01 * X0 - b1) / Q) + T * ((2.0 * a01 * X1 - b0) / Q), z)
                cb0 = torch.where(ok, S * (a11 / Q) + T * (-a01 / Q), z)
                dx = G * scale.double()[:, None, None] + md * (2.0 * xd * c00[:, None, None] + c01[:, None, None]
                                                               + yd * cb0[:, None, None])
            if terms & INVERSE:
                dx = dx * -(xd * xd)
            grad += w_reg * dx.reshape(B, -1)
    if (terms & SSI) and (terms & GRAD):
        total = out["ssi"] + alpha * out["reg"]
    else:
        total = out["ssi"] if terms & SSI else out["reg"]
    out["losses"] = torch.stack([total, out["ssi"], out["reg"]])
    if grad_losses is not None:
        out["grad"] = grad.reshape(B, H, W)
    return out


def plain_loss(pred, target, mask, terms=ALL, scales=4, image_based=True, alpha=0.1):
    """The loss written directly with differentiable torch ops in pred's dtype (autograd gives its gradient): (total, ssi,
    reg) as 0-d tensors."""
    B, H, W = pred.shape
    m = mask.bool()
    mt = m.to(pred.dtype)
    n = m.sum((1, 2))
    ssi = reg = torch.zeros((), dtype=pred.dtype)
    if terms & SSI:
        def aligned(x):
            t = x.masked_fill(~m, float("nan")).reshape(B, -1).nanmedian(-1).values
            t = torch.where(torch.isnan(t), torch.zeros_like(t), t)[:, None, None]
            s = torch.where(m, (x - t).abs(), torch.zeros_like(x)).sum((1, 2)) / (n + 1)
            return (x - t) / (s[:, None, None] + EPS)
        ssi = torch.where(m, (aligned(pred) - aligned(target)).abs(), torch.zeros_like(pred)).sum() / m.sum()
    if terms & GRAD:
        x = 1.0 / (pred + EPS) if terms & INVERSE else pred
        y = 1.0 / (target + EPS) if terms & INVERSE else target
        if terms & ALIGN:
            a00, a01, a11 = (mt * x * x).sum((1, 2)), (mt * x).sum((1, 2)), mt.sum((1, 2))
            b0, b1 = (mt * x * y).sum((1, 2)), (mt * y).sum((1, 2))
            det = a00 * a11 - a01 * a01
            ok = det != 0
            scale = torch.where(ok, (a11 * b0 - a01 * b1) / (det + EPS), torch.zeros_like(det))
            shift = torch.where(ok, (-a01 * b0 + a00 * b1) / (det + EPS), torch.zeros_like(det))
            x = scale[:, None, None] * x + shift[:, None, None]
        d = mt * (x - y)
        for k in range(scales):
            s = 2 ** k
            ds, ms = d[:, ::s, ::s], mt[:, ::s, ::s]
            img = ((ms[:, :, 1:] * ms[:, :, :-1]) * (ds[:, :, 1:] - ds[:, :, :-1]).abs()).sum((1, 2)) + \
                  ((ms[:, 1:, :] * ms[:, :-1, :]) * (ds[:, 1:, :] - ds[:, :-1, :]).abs()).sum((1, 2))
            M = ms.sum((1, 2))
            if image_based:
                reg = reg + torch.where(M != 0, img / M.clamp_min(1), img).mean()
            elif M.sum() != 0:
                reg = reg + img.sum() / M.sum()
    if (terms & SSI) and (terms & GRAD):
        return ssi + alpha * reg, ssi, reg
    return (ssi if terms & SSI else reg), ssi, reg


def assert_grad_matches_reference(got, ref, pred, mask, out, rel=1e-4):
    """got, ref [B,H,W] gradients (ref: the reference's fp32 autograd), out: forward() of the same case.  Elementwise within
    rel * max|ref| except (a) L1-kink pixels (out's ssi_kink / reg_kink: |a - g| or a pair's |dd| below 1e-5 of the values),
    at most 1e-3 of the valid pixels, where one sign may differ: a kink flip moves a pixel's gradient by twice one sign
    term, bounded by twice the image's largest |gradient|; (b) the tie set of the median (valid pixels equal to t_p, where
    the median's gradient may land on another pixel than the reference's), compared by its sum, within the image's count of
    kink pixels plus one times that jump.  Returns the number of exempted pixels."""
    got, ref = got.double(), ref.double()
    B = got.shape[0]
    gmax = ref.abs().max().item()
    tol = rel * gmax
    kink = torch.zeros_like(mask)
    for key in ("ssi_kink", "reg_kink"):
        if key in out:
            kink |= out[key] & mask
    ties = torch.zeros_like(mask)
    if "t_p" in out:
        ties = mask & (pred == out["t_p"].to(pred.dtype)[:, None, None])
    nval = int(mask.sum())
    assert int((kink & ~ties).sum()) <= max(1, 1e-3 * nval), (int(kink.sum()), nval)
    d = (got - ref).abs()
    plain = ~kink & ~ties
    assert d[plain].max().item() <= tol if plain.any() else True, (d[plain].max().item(), tol)
    for b in range(B):
        jump = 2.0 * max(ref[b].abs().max().item(), got[b].abs().max().item())
        kb = kink[b] & ~ties[b]
        if kb.any():
            assert d[b][kb].max().item() <= jump + tol, (b, d[b][kb].max().item(), jump)
        if ties[b].any():
            s = abs(got[b][ties[b]].sum().item() - ref[b][ties[b]].sum().item())
            assert s <= (int(kink[b].sum()) + 1) * jump + int(ties[b].sum()) * tol, (b, s, jump)
    return int((kink | ties).sum())
