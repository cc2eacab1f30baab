"""Virtual normal loss on the GPU, with its gradient: drop-in for omnidata_tools/torch/losses/virtual_normal_loss.py.

VNL_Loss keeps the reference's constructor and forward(gt_depth, pred_depth, select=True); the work runs in libdptx's
vnl_loss.hip (include/dptx.h dptx_vnl_*): one pass over the point triples, a radix select for the quartile cut and a
gather through an inverse index for the gradient, stream-ordered, without the reference's boolean compaction (a device-to-
host synchronisation) and sort.  The loss is differentiable with respect to either argument: the masks come from the FIRST
one, and train_depth.py passes the prediction there.  As in the reference, only delta_z and sample_ratio of the optional
constructor arguments matter (its forward hard-codes delta_cos = 0.867 and delta_diff_* = 0.005).  DepthLoss restates the
depth objective of train_depth.py:268-285.  CUDA tensors only: there is no CPU path, as everywhere in omnidata_amd.

One choice the reference leaves open: among kept triples whose loss equals the cut value, the earliest in (image, triple)
order are dropped first (the order of a stable sort).
"""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from ._native import call, check_cuda, workspace
from .engine import _stream
from .midas_loss import MidasLoss

RECORD_HEADER = 64                              # include/dptx.h DPTX_VNL_RECORD_HEADER


def _workspace(B: int, H: int, W: int, n: int, device) -> torch.Tensor:
    return workspace("dptx_vnl_workspace_bytes", device, (B, H, W, n),
                     f"unsupported virtual normal loss shape B={B} H={H} W={W} n={n} "
                     "(B >= 1, 1 <= H, W <= 8192, H*W <= 2^24, 1 <= n <= 2^29, B*n < 2^31)")


def _inputs(first, second, input_size):
    """Validates (ValueError where the reference fails or where there is no path) -> fp32 contiguous [B, H, W] tensors,
    still in the autograd graph."""
    for name, t in (("gt_depth", first), ("pred_depth", second)):
        check_cuda(name, t)
        if t.dim() != 4 or t.shape[1] != 1:
            raise ValueError(f"{name} must be [B,1,H,W], got shape {tuple(t.shape)}")
        if t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError(f"{name} must be fp32, fp16 or bf16, got {t.dtype}")
    if first.shape != second.shape or first.device != second.device:
        raise ValueError(f"shape / device mismatch: gt_depth {tuple(first.shape)} on {first.device}, pred_depth "
                         f"{tuple(second.shape)} on {second.device}")
    if tuple(first.shape[-2:]) != tuple(input_size):
        raise ValueError(f"the inputs are {tuple(first.shape[-2:])} but input_size is {tuple(input_size)}")
    B, H, W = first.shape[0], first.shape[-2], first.shape[-1]
    return first.float().reshape(B, H, W).contiguous(), second.float().reshape(B, H, W).contiguous()


def _triple_indices(p123, H: int, W: int, device) -> torch.Tensor:
    """the dict of select_index() -> int32 [3, n] linear pixel indices on the device"""
    try:
        rows = [np.asarray(p123[f"p{j}_y"]).astype(np.int64) * W + np.asarray(p123[f"p{j}_x"]).astype(np.int64) for j in (1, 2, 3)]
    except (KeyError, TypeError) as e:
        raise ValueError(f"p123 must be the dict select_index() returns: {e}") from None
    if not (rows[0].ndim == 1 and rows[0].size >= 1 and rows[0].shape == rows[1].shape == rows[2].shape):
        raise ValueError("p123 must hold six one-dimensional index arrays of one length >= 1")
    lin = np.stack(rows)
    for j in (1, 2, 3):
        x, y = np.asarray(p123[f"p{j}_x"]), np.asarray(p123[f"p{j}_y"])
        if x.min() < 0 or x.max() >= W or y.min() < 0 or y.max() >= H:
            raise ValueError(f"p123 holds an index outside the {H} x {W} image (the reference raises IndexError)")
    return torch.from_numpy(lin.astype(np.int32)).to(device)


class _VNLFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, first, second, p, fx, fy, delta_z, select):
        B, H, W = first.shape
        n = p.shape[1]
        ws = _workspace(B, H, W, n, first.device)
        loss = torch.empty((), dtype=torch.float32, device=first.device)
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        # what the backward needs belongs to this call (ctx), not to the cached workspace: two losses summed before one
        # backward() each keep their own record and inverse index
        record = torch.empty(RECORD_HEADER + B * n, dtype=torch.uint8, device=first.device) if want else None
        inverse = None
        st = _stream(first.device)
        if want:
            inverse = torch.empty(H * W + 6 * n, dtype=torch.int32, device=first.device)
            call("dptx_vnl_prepare", p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), n, H, W, inverse.data_ptr(), ws.data_ptr(),
                 ws.numel(), st)
        call("dptx_vnl_loss", first.data_ptr(), second.data_ptr(), B, H, W, fx, fy, delta_z, p[0].data_ptr(), p[1].data_ptr(),
             p[2].data_ptr(), n, int(select), loss.data_ptr(), record.data_ptr() if want else None, ws.data_ptr(), ws.numel(), st)
        ctx.cfg = (fx, fy)
        if want:
            ctx.save_for_backward(first, second, p, record, inverse)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        first, second, p, record, inverse = ctx.saved_tensors
        fx, fy = ctx.cfg
        B, H, W = first.shape
        n = p.shape[1]
        g = grad_out.float().reshape(1).contiguous()
        g1 = torch.empty_like(first) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(second) if ctx.needs_input_grad[1] else None
        call("dptx_vnl_loss_backward", first.data_ptr(), second.data_ptr(), B, H, W, fx, fy, p[0].data_ptr(), p[1].data_ptr(),
             p[2].data_ptr(), n, record.data_ptr(), inverse.data_ptr(), g.data_ptr(), g1.data_ptr() if g1 is not None else None,
             g2.data_ptr() if g2 is not None else None, _stream(first.device))
        return g1, g2, None, None, None, None, None


class VNL_Loss(torch.nn.Module):
    """VNL_Loss (:7-194): forward(gt_depth, pred_depth, select=True) on [B,1,H,W] with (H, W) == input_size -> 0-d loss,
    differentiable with respect to both arguments.  delta_cos and delta_diff_* are accepted and, as in the reference,
    never read."""

    def __init__(self, focal_x, focal_y, input_size, delta_cos=0.867, delta_diff_x=0.01, delta_diff_y=0.01, delta_diff_z=0.01,
                 delta_z=0.0001, sample_ratio=0.15):
        super().__init__()
        self.fx, self.fy = float(focal_x), float(focal_y)
        self.input_size = (int(input_size[0]), int(input_size[1]))
        self.delta_cos, self.delta_diff_x, self.delta_diff_y, self.delta_diff_z = delta_cos, delta_diff_x, delta_diff_y, delta_diff_z
        self.delta_z = delta_z
        self.sample_ratio = sample_ratio

    def select_index(self):
        """select_index (:52-72): the same calls on numpy's global generator in the same order, so np.random.seed(s) gives
        the triples the reference would draw.  Returns its dict of six arrays p{1,2,3}_{x,y}."""
        H, W = self.input_size
        num = W * H
        p123 = {}
        draws = []
        for _ in range(3):
            p = np.random.choice(num, int(num * self.sample_ratio), replace=True)
            np.random.shuffle(p)
            draws.append(p)
        for j, p in enumerate(draws, 1):
            p123[f"p{j}_x"] = p % W
            p123[f"p{j}_y"] = (p / W).astype(int)
        return p123

    def _prepared(self, gt_depth, pred_depth, p123):
        first, second = _inputs(gt_depth, pred_depth, self.input_size)
        if p123 is None:
            p123 = self.select_index()
        H, W = self.input_size
        return first, second, _triple_indices(p123, H, W, first.device)

    def forward(self, gt_depth, pred_depth, select=True, p123=None):
        """p123 (optional): the triples to use, a dict as select_index() returns; None draws them with select_index(),
        once per call, as the reference does."""
        first, second, p = self._prepared(gt_depth, pred_depth, p123)
        return _VNLFn.apply(first, second, p, self.fx, self.fy, float(self.delta_z), bool(select))

    def triples(self, gt_depth, pred_depth, p123):
        """Per-triple outputs (dptx_vnl_triples): dict of keep [B,n] bool, loss [B,n] (0 where not kept) and normal_first,
        normal_second [B,n,3].  Forward-only."""
        first, second, p = self._prepared(gt_depth.detach(), pred_depth.detach(), p123)
        B, n = first.shape[0], p.shape[1]
        H, W = self.input_size
        _workspace(B, H, W, n, first.device)   # the shape check
        keep = torch.empty(B, n, dtype=torch.uint8, device=first.device)
        loss = torch.empty(B, n, dtype=torch.float32, device=first.device)
        normals = torch.empty(B, n, 2, 3, dtype=torch.float32, device=first.device)
        call("dptx_vnl_triples", first.data_ptr(), second.data_ptr(), B, H, W, self.fx, self.fy, float(self.delta_z), p[0].data_ptr(),
             p[1].data_ptr(), p[2].data_ptr(), n, keep.data_ptr(), loss.data_ptr(), normals.data_ptr(), _stream(first.device))
        return dict(keep=keep.bool(), loss=loss, normal_first=normals[:, :, 0], normal_second=normals[:, :, 1])

    def diagnostics(self, gt_depth, pred_depth, p123, select=True):
        """The record of one forward: dict of loss (0-d tensor), K (kept triples), dropped (int(K * 0.25) with select), cut
        (the loss value at the cut) and active [B,n] bool (kept and not dropped).  Forward-only; reads the device."""
        first, second, p = self._prepared(gt_depth.detach(), pred_depth.detach(), p123)
        B, H, W = first.shape
        n = p.shape[1]
        ws = _workspace(B, H, W, n, first.device)
        loss = torch.empty(1, dtype=torch.float32, device=first.device)
        record = torch.empty(RECORD_HEADER + B * n, dtype=torch.uint8, device=first.device)
        call("dptx_vnl_loss", first.data_ptr(), second.data_ptr(), B, H, W, self.fx, self.fy, float(self.delta_z), p[0].data_ptr(),
             p[1].data_ptr(), p[2].data_ptr(), n, int(bool(select)), loss.data_ptr(), record.data_ptr(), ws.data_ptr(), ws.numel(),
             _stream(first.device))
        head = record[:16].cpu().numpy().view(np.uint32)
        return dict(loss=loss[0], K=int(head[0]), dropped=int(head[1]), cut=float(head[2:3].view(np.float32)[0]),
                    active=record[RECORD_HEADER:].view(B, n).bool())


class DepthLoss(torch.nn.Module):
    """The depth objective of train_depth.py:268-285: forward(depth_preds, depth_gt, mask_valid) on [B,1,H,W] -> dict of
    ssi_loss, reg_loss, vn_loss and depth_loss = ssi_loss + alpha * reg_loss + vnl_weight * vn_loss.  MidasLoss(alpha) gives ssi_loss and
    reg_loss; vn_loss = VNL_Loss(1.0, 1.0, (image_size, image_size))(depth_preds, depth_gt): the prediction goes FIRST."""

    def __init__(self, alpha=0.1, vnl_weight=10.0, image_size=384):
        super().__init__()
        self.alpha = alpha
        self.vnl_weight = vnl_weight
        self.midas_loss = MidasLoss(alpha=alpha)
        self.vnl_loss = VNL_Loss(1.0, 1.0, (image_size, image_size))

    def forward(self, depth_preds, depth_gt, mask_valid):
        _, ssi_loss, reg_loss = self.midas_loss(depth_preds, depth_gt, mask_valid)
        vn_loss = self.vnl_loss(depth_preds, depth_gt)
        loss = ssi_loss + self.alpha * reg_loss + self.vnl_weight * vn_loss
        return {"ssi_loss": ssi_loss, "reg_loss": reg_loss, "vn_loss": vn_loss, "depth_loss": loss}
