"""Surface-normal training loss on the GPU, with its gradient: drop-in for omnidata_tools/torch/losses/masked_losses.py and
the objective of train_normal.py:205-265.

masked_l1_loss / masked_mse_loss / masked_loss / masked_cosine_angular_loss keep the reference's names and signatures,
make_valid_mask is the method of train_normal.py (train_depth.py has the same one), and NormalLoss restates
train_normal.py:251-265: the prediction clamped to [0, 1], cos_loss + 10 * l1_loss.  The work runs in libdptx's
normal_loss.hip (include/dptx.h dptx_normal_*, dptx_masked_*, dptx_valid_mask): one streaming pass forward and one backward,
stream-ordered, without the reference's boolean compaction (a device-to-host synchronisation) and its [B,3,H,W]
temporaries.  Everything is differentiable with respect to the prediction only.  CUDA tensors only: there is no CPU path,
as everywhere in omnidata_amd.

Numerics: per-pixel fp32 values rounded as the reference's fp32 tensors, fp64 sums in a fixed order (bitwise reproducible).
An empty mask gives NaN (masked_loss: 0) and an all-zero gradient, as the reference does.
"""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from ._native import call, check_cuda, workspace
from .engine import _stream, load_library

L1, COS, CLAMP_PRED = 1, 2, 4                   # include/dptx.h DPTX_NORMAL_*
RECORD_DOUBLES = 1                              # DPTX_NORMAL_RECORD_DOUBLES: the count of the mask
MASKED_L1, MASKED_MSE, MASKED_VALUE, MASKED_EMPTY_ZERO = 0, 1, 2, 4   # DPTX_MASKED_*
_FLOATS = (torch.float32, torch.float16, torch.bfloat16)


def _unsupported(B: int, H: int, W: int) -> str:
    return f"unsupported normal loss shape B={B} H={H} W={W} (B >= 1, 1 <= H, W <= 8192, H*W <= 2^24)"


def _workspace(B: int, H: int, W: int, device) -> torch.Tensor:
    return workspace("dptx_normal_workspace_bytes", device, (B, H, W), _unsupported(B, H, W))


def _check_shape(B: int, H: int, W: int) -> None:
    """ValueError for a shape the entry points reject, for the kernels that take no workspace: nothing is allocated."""
    if load_library().dptx_normal_workspace_bytes(B, H, W, ctypes.byref(ctypes.c_int64())) != 0:
        raise ValueError(_unsupported(B, H, W))


def _check_float(name, t):
    check_cuda(name, t)
    if t.dtype not in _FLOATS:
        raise ValueError(f"{name} must be fp32, fp16 or bf16, got {t.dtype}")


def _check_target(target):
    if target.requires_grad:
        raise ValueError("target must not require grad (the gradient is with respect to the prediction only)")


def _normal_inputs(preds, target, mask_valid):
    """Validates -> fp32 contiguous prediction [B,3,H,W] (still in the autograd graph) and target, uint8 mask [B,H,W]
    (channel 0 of the given one, as the reference's cosine loss reads it)."""
    for name, t in (("preds", preds), ("target", target)):
        _check_float(name, t)
        if t.dim() != 4 or t.shape[1] != 3:
            raise ValueError(f"{name} must be [B,3,H,W], got shape {tuple(t.shape)}")
    check_cuda("mask_valid", mask_valid)
    B, _, H, W = preds.shape
    if mask_valid.dim() != 4 or mask_valid.shape[1] not in (1, 3) or (mask_valid.shape[0], *mask_valid.shape[2:]) != (B, H, W):
        raise ValueError(f"mask_valid must be [B,1,H,W] or [B,3,H,W] for preds {tuple(preds.shape)}, got shape "
                         f"{tuple(mask_valid.shape)}")
    if preds.shape != target.shape or not (preds.device == target.device == mask_valid.device):
        raise ValueError(f"shape / device mismatch: preds {tuple(preds.shape)} on {preds.device}, target {tuple(target.shape)} on "
                         f"{target.device}, mask_valid on {mask_valid.device}")
    _check_target(target)
    m = mask_valid[:, 0].bool().contiguous().view(torch.uint8)
    return preds.float().contiguous(), target.detach().float().contiguous(), m


class _NormalLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, mask, flags, l1_weight):
        B, _, H, W = pred.shape
        ws = _workspace(B, H, W, pred.device)
        losses = torch.empty(3, dtype=torch.float32, device=pred.device)
        want = ctx.needs_input_grad[0]
        # the record belongs to this call (ctx), not to the cached workspace: two losses summed before one backward() each
        # keep their own
        record = torch.empty(RECORD_DOUBLES, dtype=torch.float64, device=pred.device) if want else None
        call("dptx_normal_loss", pred.data_ptr(), target.data_ptr(), mask.data_ptr(), B, H, W, flags, float(l1_weight),
             losses.data_ptr(), record.data_ptr() if want else None, ws.data_ptr(), ws.numel(), _stream(pred.device))
        ctx.cfg = (flags, float(l1_weight))
        if want:
            ctx.save_for_backward(pred, target, mask, record)
        return losses

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_losses):
        pred, target, mask, record = ctx.saved_tensors
        flags, l1_weight = ctx.cfg
        B, _, H, W = pred.shape
        g = grad_losses.float().contiguous()
        grad = torch.empty_like(pred)
        call("dptx_normal_loss_backward", pred.data_ptr(), target.data_ptr(), mask.data_ptr(), B, H, W, flags, l1_weight,
             record.data_ptr(), g.data_ptr(), grad.data_ptr(), _stream(pred.device))
        return grad, None, None, None, None


class _MaskedLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, mask, kind):
        n = pred.numel()
        ws = workspace("dptx_masked_workspace_bytes", pred.device, (n,), f"unsupported masked loss size n={n} (1 <= n <= 2^40)")
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        want = ctx.needs_input_grad[0]
        record = torch.empty(1, dtype=torch.float64, device=pred.device) if want else None
        call("dptx_masked_loss", pred.data_ptr(), target.data_ptr() if target is not None else None, mask.data_ptr(), n, kind,
             loss.data_ptr(), record.data_ptr() if want else None, ws.data_ptr(), ws.numel(), _stream(pred.device))
        ctx.kind = kind
        ctx.has_target = target is not None
        if want:
            ctx.save_for_backward(pred, mask, record, *((target,) if target is not None else ()))
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        pred, mask, record = ctx.saved_tensors[:3]
        target = ctx.saved_tensors[3] if ctx.has_target else None
        g = grad_loss.float().reshape(1).contiguous()
        grad = torch.empty_like(pred)
        call("dptx_masked_loss_backward", pred.data_ptr(), target.data_ptr() if target is not None else None, mask.data_ptr(),
             pred.numel(), ctx.kind, record.data_ptr(), g.data_ptr(), grad.data_ptr(), _stream(pred.device))
        return grad, None, None, None


def _masked(preds, target, mask_valid, kind):
    _check_float("preds", preds)
    check_cuda("mask_valid", mask_valid)
    if target is not None:
        _check_float("target", target)
        _check_target(target)
        if target.shape != preds.shape or target.device != preds.device:
            raise ValueError(f"shape / device mismatch: preds {tuple(preds.shape)} on {preds.device}, target "
                             f"{tuple(target.shape)} on {target.device}")
    if mask_valid.dtype != torch.bool:
        raise ValueError(f"mask_valid must be a bool tensor, got {mask_valid.dtype} (the reference's ~mask_valid needs one)")
    if mask_valid.shape != preds.shape or mask_valid.device != preds.device:
        raise ValueError(f"mask_valid must have the shape and device of preds, {tuple(preds.shape)} on {preds.device}, got "
                         f"{tuple(mask_valid.shape)} on {mask_valid.device}")
    if preds.numel() == 0:
        raise ValueError("preds must not be empty")
    t = target.detach().float().contiguous() if target is not None else None
    return _MaskedLossFn.apply(preds.float().contiguous(), t, mask_valid.contiguous().view(torch.uint8), kind)


def masked_l1_loss(preds, target, mask_valid):
    """masked_l1_loss (:4-7): sum of |preds - target| over the bool mask (a mask per element, the shape of preds) divided by
    its count; 0-d, differentiable with respect to preds.  An empty mask gives NaN."""
    return _masked(preds, target, mask_valid, MASKED_L1)


def masked_mse_loss(preds, target, mask_valid):
    """masked_mse_loss (:9-12): the same with (preds - target) ** 2."""
    return _masked(preds, target, mask_valid, MASKED_MSE)


def masked_loss(element_wise_loss, mask_valid):
    """masked_loss (:26-30): sum of element_wise_loss over the mask divided by its count, 0 for an empty mask (decided on the
    device: no host read).  The reference's in-place side effect -- it zeroes its argument outside the mask -- is NOT
    reproduced: element_wise_loss is left as it is."""
    return _masked(element_wise_loss, None, mask_valid, MASKED_VALUE | MASKED_EMPTY_ZERO)


def masked_cosine_angular_loss(preds, target, mask_valid):
    """masked_cosine_angular_loss (:14-23) on [B,3,H,W] with a mask [B,1 or 3,H,W] of which channel 0 is used, as in the
    reference: the mean over the valid pixels of -cos of the angle between 2 preds - 1 and 2 target - 1 (each clamped to
    [-1, 1]); 0-d, differentiable with respect to preds."""
    p, t, m = _normal_inputs(preds, target, mask_valid)
    return _NormalLossFn.apply(p, t, m, COS, 0.0)[2]


def make_valid_mask(mask_float, max_pool_size=4):
    """make_valid_mask (train_normal.py:205-232) of a 2-D [H,W], 3-D [C,H,W] or 4-D [B,1,H,W] mask as the Taskonomy loader
    gives it -> [B,1,H,W] bool: valid where max_pool2d(1 - mask, max_pool_size), resized back with 'nearest', is exactly 0.
    The 5-D form of the reference is not supported."""
    check_cuda("mask_float", mask_float)
    if mask_float.dim() == 3:
        mask_float = mask_float.unsqueeze(0)
    elif mask_float.dim() == 2:
        mask_float = mask_float.unsqueeze(0).unsqueeze(0)
    if mask_float.dim() != 4:
        raise ValueError(f"mask_float must be 2-D, 3-D or 4-D, got shape {tuple(mask_float.shape)} (the 5-D form is not supported)")
    if not mask_float.is_floating_point():
        raise ValueError(f"mask_float must be a floating-point tensor, got {mask_float.dtype}")
    pool = int(max_pool_size)
    B, C, H, W = mask_float.shape
    if B * C < 1 or pool < 1 or H < pool or W < pool:
        raise ValueError(f"unsupported mask shape {tuple(mask_float.shape)} for max_pool_size={max_pool_size} (H, W >= max_pool_size >= 1)")
    _check_shape(B * C, H, W)
    m = mask_float.detach().float().contiguous()
    valid = torch.empty(B, C, H, W, dtype=torch.uint8, device=m.device)
    call("dptx_valid_mask", m.data_ptr(), B * C, H, W, pool, valid.data_ptr(), _stream(m.device))
    return valid.view(torch.bool)


class NormalLoss(torch.nn.Module):
    """The normal objective of train_normal.py:251-265: forward(normal_preds, normal_gt, mask_valid) on [B,3,H,W] with a
    [B,1,H,W] or [B,3,H,W] bool mask (channel 0 is used for both terms: the reference's repeat_interleave(3, 1) of a
    one-channel mask) -> dict of l1_loss, cos_loss and normal_loss = cos_loss + l1_weight * l1_loss, 0-d tensors,
    differentiable with respect to the prediction.  clamp_pred: the prediction is clamped to [0, 1] first (:251), and the
    gradient goes through the clamp.  One forward launch pair and one backward launch."""

    def __init__(self, l1_weight=10.0, clamp_pred=True):
        super().__init__()
        self.l1_weight = float(l1_weight)
        self.clamp_pred = bool(clamp_pred)

    def _flags(self):
        return CLAMP_PRED if self.clamp_pred else 0

    def forward(self, normal_preds, normal_gt, mask_valid):
        p, t, m = _normal_inputs(normal_preds, normal_gt, mask_valid)
        out = _NormalLossFn.apply(p, t, m, L1 | COS | self._flags(), self.l1_weight)
        return {"l1_loss": out[1], "cos_loss": out[2], "normal_loss": out[0]}

    def pixels(self, normal_preds, normal_gt, mask_valid):
        """Per-pixel terms (dptx_normal_pixels): (cos, l1), each [B,H,W] fp32 and 0 outside the mask; cos is the pixel's
        -cos, l1 the sum of its three |p - t|.  Forward-only."""
        p, t, m = _normal_inputs(normal_preds.detach(), normal_gt, mask_valid)
        B, _, H, W = p.shape
        _check_shape(B, H, W)
        cos = torch.empty(B, H, W, dtype=torch.float32, device=p.device)
        l1 = torch.empty(B, H, W, dtype=torch.float32, device=p.device)
        call("dptx_normal_pixels", p.data_ptr(), t.data_ptr(), m.data_ptr(), B, H, W, self._flags(), cos.data_ptr(), l1.data_ptr(),
             _stream(p.device))
        return cos, l1
