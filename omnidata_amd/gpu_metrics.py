"""Evaluation metrics on the GPU: paper_code/evaluation_metrics.py:13-106 (get_metrics for task 'normal' and
'depth_zbuffer') without leaving the device.

omnidata_amd.metrics restates the reference with torch ops and reads about ten scalars back per call; here the work runs in
libdptx's eval_metrics.hip (include/dptx.h dptx_eval_*): one streaming pass, the exact median by a radix select, fp64 sums
in a fixed order, stream-ordered, no synchronisation and no [B*H*W, 3] temporaries.  One call gives the reference's row for
the whole batch, or with per_image one row per image (what the reference's test scripts compute with one call per image).

    normal_metrics(pred, target, mask, per_image=False)  ->  dict of fp64 CUDA tensors, 0-d or [B]
    depth_metrics(pred, target, mask, per_image=False)   ->  the same for depth
    get_metrics(pred, target, task=None, masks=None)     ->  the reference's shape: dict of floats or None, one copy
    MetricsAccumulator(task)                             ->  mean and std over the images of a dataset
    normal_angles(pred, target)                          ->  [B,H,W] fp64: every pixel's angular error in degrees

Key names are those of omnidata_amd.metrics plus num_valid.  pred / target: [B,3,H,W] (normal) or [B,1,H,W] (depth) in fp32,
fp16 or bf16; mask: [B, 1 or C, H, W] bool, of which channel 0 is used, as in the reference.  CUDA tensors only: there is no
CPU path, as everywhere in omnidata_amd.

The workspace is cached per (device, shape) for the life of the process, as in the other wrappers of libdptx, and is shared
by both tasks (the depth kernels leave its 8 B / pixel key region untouched).  Calls of one shape must therefore follow one
another on one stream at a time; two streams that evaluate the same shape concurrently would race on it.

Two things differ from omnidata_amd.metrics, both on the reference's side: a NaN angle among the valid pixels makes
ang_error_median NaN (np.median propagates it), and an empty mask gives num_valid = 0 and NaN elsewhere instead of None
(get_metrics here returns None, after its one copy).
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional

import torch

from ._native import call, check_cuda, workspace
from .engine import _stream, load_library

__all__ = ["normal_metrics", "depth_metrics", "get_metrics", "normal_angles", "MetricsAccumulator", "NORMAL_FIELDS", "DEPTH_FIELDS"]

PER_IMAGE = 1                                   # include/dptx.h DPTX_EVAL_PER_IMAGE
# the rows of dptx_eval_normal / dptx_eval_depth (DPTX_EVAL_NORMAL_FIELDS, DPTX_EVAL_DEPTH_FIELDS), in order
NORMAL_FIELDS = ("num_valid", "ang_error_mean", "ang_error_median", "ang_error_without_masking", "percentage_within_11.25_degrees",
                 "percentage_within_22.5_degrees", "percentage_within_30_degrees", "eval_L1", "eval_mse")
DEPTH_FIELDS = ("num_valid", "eval_L1", "eval_mse", "log10_diff", "log10", "si_log", "rel_error", "irmse")
_TASKS = {"normal": ("dptx_eval_normal", 3, NORMAL_FIELDS), "depth_zbuffer": ("dptx_eval_depth", 1, DEPTH_FIELDS)}
_FLOATS = (torch.float32, torch.float16, torch.bfloat16)


def _task(task):
    if task not in _TASKS:
        raise ValueError(f"task must be 'normal' or 'depth_zbuffer', got {task!r}")
    return _TASKS[task]


def _pair(pred, target, channels):
    """Validates -> fp32 contiguous pred and target [B,C,H,W]."""
    for name, t in (("pred", pred), ("target", target)):
        check_cuda(name, t)
        if t.dtype not in _FLOATS:
            raise ValueError(f"{name} must be fp32, fp16 or bf16, got {t.dtype}")
        if t.dim() != 4 or t.shape[1] != channels:
            raise ValueError(f"{name} must be [B,{channels},H,W], got shape {tuple(t.shape)}")
    if pred.shape != target.shape or pred.device != target.device:
        raise ValueError(f"shape / device mismatch: pred {tuple(pred.shape)} on {pred.device}, target {tuple(target.shape)} on "
                         f"{target.device}")
    if pred.numel() == 0:
        raise ValueError("pred must not be empty")
    return pred.detach().float().contiguous(), target.detach().float().contiguous()


def _inputs(pred, target, mask, channels):
    """Validates -> fp32 contiguous pred, target [B,C,H,W] and the uint8 mask [B,H,W] (channel 0 of the given one)."""
    p, t = _pair(pred, target, channels)
    check_cuda("mask", mask)
    if mask.dtype != torch.bool:
        raise ValueError(f"mask must be a bool tensor, got {mask.dtype}")
    B, _, H, W = p.shape
    if mask.dim() != 4 or mask.shape[1] not in (1, channels) or (mask.shape[0], *mask.shape[2:]) != (B, H, W) or mask.device != p.device:
        raise ValueError(f"mask must be [B,1,H,W] or [B,{channels},H,W] on {p.device} for pred {tuple(p.shape)}, got shape "
                         f"{tuple(mask.shape)} on {mask.device}")
    return p, t, mask[:, 0].contiguous().view(torch.uint8)


def _unsupported(B: int, H: int, W: int) -> str:
    return f"unsupported metrics shape B={B} H={H} W={W} (B >= 1, 1 <= H, W <= 8192, H*W <= 2^24, B*H*W < 2^32)"


def _rows(task, pred, target, mask, per_image):
    """-> fp64 CUDA tensor [rows, fields], rows = B with per_image, else 1; stream-ordered, no synchronisation."""
    entry, channels, fields = _task(task)
    p, t, m = _inputs(pred, target, mask, channels)
    B, _, H, W = p.shape
    ws = workspace("dptx_eval_workspace_bytes", p.device, (B, H, W), _unsupported(B, H, W))
    out = torch.empty(B if per_image else 1, len(fields), dtype=torch.float64, device=p.device)
    call(entry, p.data_ptr(), t.data_ptr(), m.data_ptr(), B, H, W, PER_IMAGE if per_image else 0, out.data_ptr(), ws.data_ptr(),
         ws.numel(), _stream(p.device))
    return out


def _as_dict(rows, fields, per_image) -> Dict[str, torch.Tensor]:
    return {name: (rows[:, k] if per_image else rows[0, k]) for k, name in enumerate(fields)}


def normal_metrics(pred, target, mask, per_image: bool = False) -> Dict[str, torch.Tensor]:
    """The metrics of task 'normal' (:33-59, :88-96) as fp64 CUDA tensors, 0-d for the whole batch or [B] with per_image (row i
    is what the reference returns for image i alone).  An empty mask gives num_valid 0 and NaN elsewhere.  No
    synchronisation."""
    return _as_dict(_rows("normal", pred, target, mask, per_image), NORMAL_FIELDS, per_image)


def depth_metrics(pred, target, mask, per_image: bool = False) -> Dict[str, torch.Tensor]:
    """The metrics of task 'depth_zbuffer' (:61-79, :97-104), as normal_metrics."""
    return _as_dict(_rows("depth_zbuffer", pred, target, mask, per_image), DEPTH_FIELDS, per_image)


def normal_angles(pred, target) -> torch.Tensor:
    """The angular error of every pixel in degrees (:36-43), [B,H,W] fp64, the mask not applied (dptx_eval_normal_pixels):
    the values whose masked mean, median and threshold counts normal_metrics reports."""
    p, t = _pair(pred, target, 3)
    B, _, H, W = p.shape
    if load_library().dptx_eval_workspace_bytes(B, H, W, ctypes.byref(ctypes.c_int64())) != 0:   # no workspace: nothing allocated
        raise ValueError(_unsupported(B, H, W))
    ang = torch.empty(B, H, W, dtype=torch.float64, device=p.device)
    call("dptx_eval_normal_pixels", p.data_ptr(), t.data_ptr(), B, H, W, ang.data_ptr(), _stream(p.device))
    return ang


def get_metrics(pred, target, task=None, masks=None) -> Optional[Dict[str, float]]:
    """Reference-shaped entry point (:13): task in {'normal', 'depth_zbuffer'} -> dict of Python floats with the reference's
    keys, or None for an empty mask; one device-to-host copy of the row.  Any other task (the reference's task-less L1 / MSE
    included) raises ValueError."""
    _, _, fields = _task(task)
    row = _rows(task, pred, target, masks, False)[0].cpu().tolist()
    if row[0] < 1.0:
        return None
    return dict(zip(fields[1:], row[1:]))


class MetricsAccumulator:
    """Mean and standard deviation of every metric over the images of a dataset, as the reference's test scripts print them
    (paper_code/test_normal.py:455-457: one get_metrics call per image, a running mean and variance per metric).

    update(pred, target, mask) adds the per-image rows of a batch to running sums on the device (count, sum and sum of
    squares per field, images with an empty mask left out, as the reference skips a None); plain torch ops, no
    synchronisation.  compute() makes one copy and returns {name: (mean, std)}, with num_images the number of images that
    counted.  std is the SAMPLE standard deviation (divisor n - 1, what runstats' Statistics.variance() gives there), from
    the sums: sqrt(max(sumsq - sum^2 / n, 0) / (n - 1)); NaN for n < 2, and mean NaN for n == 0."""

    def __init__(self, task: str):
        _, _, self.fields = _task(task)
        self.task = task
        self._acc = None   # fp64 [3, fields]: count, sum, sum of squares

    def update(self, pred, target, mask) -> None:
        rows = _rows(self.task, pred, target, mask, True)
        if self._acc is None:
            self._acc = torch.zeros(3, len(self.fields), dtype=torch.float64, device=rows.device)
        keep = rows[:, :1] > 0
        kept = torch.where(keep, rows, torch.zeros_like(rows))
        self._acc += torch.stack([keep.double().expand_as(rows).sum(0), kept.sum(0), (kept * kept).sum(0)])

    def compute(self) -> Dict[str, tuple]:
        if self._acc is None:
            raise RuntimeError("MetricsAccumulator.compute() before any update()")
        cnt, s, ss = self._acc.cpu().tolist()
        out = {}
        for k, name in enumerate(self.fields):
            n = cnt[k]
            mean = s[k] / n if n > 0 else math.nan
            std = math.sqrt(max(ss[k] - s[k] * s[k] / n, 0.0) / (n - 1)) if n > 1 else math.nan
            out[name] = (mean, std)
        out["num_images"] = int(cnt[0])
        return out
