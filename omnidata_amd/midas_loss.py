"""MiDaS depth loss on the GPU, with its gradient: drop-in for omnidata_tools/torch/losses/midas_loss.py.

The depth-training loss of the reference (train_depth.py): a scale-and-shift-invariant MAE (SSIMAE) plus a multi-scale
gradient-matching term on the least-squares aligned inverse depth.  MidasLoss / SSIMAE / GradientMatchingTerm /
compute_scale_and_shift / masked_shift_and_scale keep the reference's names and signatures; the work runs in libdptx's
midas_loss.hip (include/dptx.h dptx_midas_*).  The loss modules are differentiable with respect to the prediction; the two
alignment functions are forward-only.  CUDA tensors only: there is no CPU path, as everywhere in omnidata_amd.

Numerics: per-pixel fp32 values rounded as the reference's fp32 tensors, fp64 sums and 2x2 solve.  One deliberate
difference: where the alignment's det is exactly 0 (a constant prediction on the mask), scale = shift = 0; the reference's
fp32 sums leave a tiny non-zero det there and an arbitrary scale.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from ._native import call, check_cuda, workspace
from .engine import _stream

SSI, GRAD, ALIGN, INVERSE = 1, 2, 4, 8          # include/dptx.h DPTX_MIDAS_*
RECORD_DOUBLES = 32                             # DPTX_MIDAS_RECORD_DOUBLES
STATS = 8                                       # DPTX_MIDAS_STATS


def _workspace(B: int, H: int, W: int, scales: int, device) -> torch.Tensor:
    return workspace("dptx_midas_workspace_bytes", device, (B, H, W, scales),
                     f"unsupported MiDaS loss shape B={B} H={H} W={W} scales={scales} "
                     "(B >= 1, 1 <= H, W <= 8192, H*W <= 2^24, 1 <= scales <= 8)")


def _inputs(prediction, target, mask, dim: int, differentiable: bool):
    """Validates (ValueError where the reference raises or where there is no path) -> fp32 prediction (still in the autograd
    graph), fp32 target and uint8 mask, contiguous [B, H, W]."""
    shape = "[B,1,H,W]" if dim == 4 else "[B,H,W]"
    for name, t in (("prediction", prediction), ("target", target), ("mask", mask)):
        check_cuda(name, t)
        if t.dim() != dim or (dim == 4 and t.shape[1] != 1):
            raise ValueError(f"{name} must be {shape}, got shape {tuple(t.shape)}")
    if prediction.shape != target.shape or mask.shape != prediction.shape:
        raise ValueError(f"shape mismatch: prediction {tuple(prediction.shape)}, target {tuple(target.shape)}, "
                         f"mask {tuple(mask.shape)}")
    if mask.dtype != torch.bool:
        raise ValueError(f"mask must be a bool tensor, got {mask.dtype} (the reference's ~mask raises TypeError)")
    for name, t in (("prediction", prediction), ("target", target)):
        if t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError(f"{name} must be fp32, fp16 or bf16, got {t.dtype}")
    if target.requires_grad:
        raise ValueError("target must not require grad (the gradient is with respect to the prediction only)")
    if not differentiable and prediction.requires_grad and torch.is_grad_enabled():
        raise ValueError("this function is forward-only; MidasLoss / SSIMAE / GradientMatchingTerm give gradients")
    B, H, W = prediction.shape[0], prediction.shape[-2], prediction.shape[-1]
    p = prediction.float().reshape(B, H, W).contiguous()
    t = target.detach().float().reshape(B, H, W).contiguous()
    m = mask.reshape(B, H, W).contiguous().view(torch.uint8)
    return p, t, m


class _MidasLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, mask, terms, scales, image_based, alpha):
        B, H, W = pred.shape
        ws = _workspace(B, H, W, scales, pred.device)
        losses = torch.empty(3, dtype=torch.float32, device=pred.device)
        want = ctx.needs_input_grad[0]
        # the coefficient record belongs to this call (ctx), not to the cached workspace: two losses summed before one
        # backward() each keep their own
        record = torch.empty(B, RECORD_DOUBLES, dtype=torch.float64, device=pred.device) if want else None
        call("dptx_midas_loss", pred.data_ptr(), target.data_ptr(), mask.data_ptr(), B, H, W, terms, scales, int(image_based),
             float(alpha), losses.data_ptr(), record.data_ptr() if want else None, ws.data_ptr(), ws.numel(), _stream(pred.device))
        ctx.cfg = (terms, scales, int(image_based), float(alpha))
        if want:
            ctx.save_for_backward(pred, target, mask, record)
        return losses

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_losses):
        pred, target, mask, record = ctx.saved_tensors
        terms, scales, image_based, alpha = ctx.cfg
        B, H, W = pred.shape
        g = grad_losses.float().contiguous()
        grad = torch.empty_like(pred)
        call("dptx_midas_loss_backward", pred.data_ptr(), target.data_ptr(), mask.data_ptr(), B, H, W, terms, scales, image_based,
             alpha, record.data_ptr(), g.data_ptr(), grad.data_ptr(), _stream(pred.device))
        return grad, None, None, None, None, None, None


def _loss(prediction, target, mask, dim, terms, scales, image_based, alpha):
    p, t, m = _inputs(prediction, target, mask, dim, differentiable=True)
    return _MidasLossFn.apply(p, t, m, terms, int(scales), image_based, alpha)


class SSIMAE(torch.nn.Module):
    """SSIMAE (:104-111): forward(depth_preds, depth_gt, mask_valid) on [B,1,H,W] -> 0-d scale-and-shift-invariant MAE."""

    def forward(self, depth_preds, depth_gt, mask_valid):
        return _loss(depth_preds, depth_gt, mask_valid, 4, SSI, 1, True, 1.0)[1]


class GradientMatchingTerm(torch.nn.Module):
    """GradientMatchingTerm (:114-134) on [B,H,W] raw values; any reduction other than 'batch-based' is image-based."""

    def __init__(self, scales=4, reduction='batch-based'):
        super().__init__()
        self.scales = int(scales)
        self.image_based = reduction != 'batch-based'

    def forward(self, prediction, target, mask):
        return _loss(prediction, target, mask, 3, GRAD, self.scales, self.image_based, 1.0)[2]


class MidasLoss(torch.nn.Module):
    """MidasLoss (:137-157): forward(prediction, target, mask) on [B,1,H,W] -> (total, ssi_loss, reg_loss), 0-d tensors,
    total = ssi_loss + alpha * reg_loss, differentiable with respect to the prediction.  alpha <= 0 raises ValueError at
    forward (the reference raises UnboundLocalError there)."""

    def __init__(self, alpha=0.1, scales=4, reduction='image-based'):
        super().__init__()
        self.alpha = alpha
        self.scales = int(scales)
        self.image_based = reduction != 'batch-based'

    def forward(self, prediction, target, mask):
        if not self.alpha > 0:
            raise ValueError(f"alpha must be > 0, got {self.alpha} (the reference's forward raises)")
        out = _loss(prediction, target, mask, 4, SSI | GRAD | ALIGN | INVERSE, self.scales, self.image_based, self.alpha)
        return out[0], out[1], out[2]


def _stats(prediction, target, mask, dim, terms, aligned=False):
    p, t, m = _inputs(prediction, target, mask, dim, differentiable=False)
    B, H, W = p.shape
    ws = _workspace(B, H, W, 1, p.device)
    st = torch.empty(B, STATS, dtype=torch.float32, device=p.device)
    pa = torch.empty_like(p) if aligned else None
    ga = torch.empty_like(t) if aligned else None
    call("dptx_midas_stats", p.data_ptr(), t.data_ptr(), m.data_ptr(), B, H, W, terms, st.data_ptr(),
         pa.data_ptr() if aligned else None, ga.data_ptr() if aligned else None, ws.data_ptr(), ws.numel(), _stream(p.device))
    return st, pa, ga


def compute_scale_and_shift(prediction, target, mask):
    """compute_scale_and_shift (:10-30) on [B,H,W] with a bool mask -> (scale [B], shift [B]); forward-only."""
    st, _, _ = _stats(prediction, target, mask, 3, ALIGN)
    return st[:, 5].clone(), st[:, 6].clone()


def masked_shift_and_scale(depth_preds, depth_gt, mask_valid):
    """masked_shift_and_scale (:33-56) on [B,1,H,W] -> (depth_pred_aligned, depth_gt_aligned); forward-only."""
    _, pa, ga = _stats(depth_preds, depth_gt, mask_valid, 4, SSI, aligned=True)
    return pa.view(depth_preds.shape), ga.view(depth_gt.shape)


def alignment_stats(prediction, target, mask):
    """The per-image statistics MidasLoss uses, on [B,1,H,W]: dict of [B] tensors t_p, t_g (lower nanmedians, 0 without a
    non-NaN valid value), s_p, s_g, n (valid pixels), scale, shift (the alignment of the inverse depths) and argmedian (the
    linear index the median's gradient flows to, -1: none)."""
    st, _, _ = _stats(prediction, target, mask, 4, SSI | ALIGN | INVERSE)
    names = ("t_p", "t_g", "s_p", "s_g", "n", "scale", "shift")
    out = {k: st[:, i].clone() for i, k in enumerate(names)}
    out["n"] = out["n"].long()
    out["argmedian"] = st[:, 7].long()
    return out
