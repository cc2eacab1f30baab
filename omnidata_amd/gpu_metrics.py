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
    aligned_depth_metrics(pred, target, mask, align=...) ->  depth metrics of the prediction fitted to the target per image
    align_depth(pred, target, mask, align)               ->  the fitted prediction and its (scale, shift) per image

The depth network's output is defined up to a scale and a shift per image, so a depth checkpoint is judged after a per-image
fit to the ground truth: align='lstsq' (compute_scale_and_shift, losses/midas_loss.py:10-30) or align='median'
(masked_shift_and_scale, :33-56).  dptx_eval_depth_aligned fits, aligns and evaluates in one call and adds the standard
benchmark fields abs_rel, sq_rel, rmse, rmse_log and delta1..3; get_metrics and MetricsAccumulator take align= and go
through it, and without it they are the unaligned code path.

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

__all__ = ["normal_metrics", "depth_metrics", "get_metrics", "normal_angles", "MetricsAccumulator", "NORMAL_FIELDS", "DEPTH_FIELDS",
           "aligned_depth_metrics", "align_depth", "ALIGNED_DEPTH_FIELDS"]

PER_IMAGE = 1                                   # include/dptx.h DPTX_EVAL_PER_IMAGE
# the rows of dptx_eval_normal / dptx_eval_depth (DPTX_EVAL_NORMAL_FIELDS, DPTX_EVAL_DEPTH_FIELDS), in order
NORMAL_FIELDS = ("num_valid", "ang_error_mean", "ang_error_median", "ang_error_without_masking", "percentage_within_11.25_degrees",
                 "percentage_within_22.5_degrees", "percentage_within_30_degrees", "eval_L1", "eval_mse")
DEPTH_FIELDS = ("num_valid", "eval_L1", "eval_mse", "log10_diff", "log10", "si_log", "rel_error", "irmse")
# the rows of dptx_eval_depth_aligned (DPTX_EVAL_ALIGNED_FIELDS)
ALIGNED_DEPTH_FIELDS = DEPTH_FIELDS + ("abs_rel", "sq_rel", "rmse", "rmse_log", "delta1", "delta2", "delta3")
_ALIGN = {"lstsq": 1, "median": 2}               # DPTX_EVAL_ALIGN_LSTSQ, DPTX_EVAL_ALIGN_MEDIAN
ALIGNED_CLAMP = 1                                # DPTX_EVAL_ALIGNED_CLAMP
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


def _check_align(task, align, min_depth=1e-3):
    _task(task)
    if align not in _ALIGN:
        raise ValueError(f"align must be one of {sorted(_ALIGN)}, got {align!r}")
    if task != "depth_zbuffer":
        raise ValueError(f"align={align!r} needs task='depth_zbuffer': there is no aligned evaluation of task {task!r}")
    try:   # the C ABI takes a float: judge the value it will see (1e-50 is 0.0f there, 1e39 is inf)
        md = float(torch.tensor(float(min_depth), dtype=torch.float64).float())
    except (TypeError, ValueError):
        md = math.nan
    if not (math.isfinite(md) and md > 0):
        raise ValueError(f"min_depth must be positive and finite as an fp32 number, got {min_depth!r}")


def _aligned_rows(pred, target, mask, align, clamp, min_depth, want_aligned=False):
    """-> (rows fp64 [B + 1, 15], coeffs fp32 [B, 2], aligned fp32 [B,1,H,W] or None); stream-ordered, no synchronisation."""
    _check_align("depth_zbuffer", align, min_depth)
    p, t, m = _inputs(pred, target, mask, 1)
    B, _, H, W = p.shape
    ws = workspace("dptx_eval_aligned_workspace_bytes", p.device, (B, H, W), _unsupported(B, H, W))
    out = torch.empty(B + 1, len(ALIGNED_DEPTH_FIELDS), dtype=torch.float64, device=p.device)
    coeffs = torch.empty(B, 2, dtype=torch.float32, device=p.device)
    al = torch.empty_like(p) if want_aligned else None
    call("dptx_eval_depth_aligned", p.data_ptr(), t.data_ptr(), m.data_ptr(), B, H, W, _ALIGN[align], ALIGNED_CLAMP if clamp else 0,
         float(min_depth), out.data_ptr(), coeffs.data_ptr(), al.data_ptr() if want_aligned else None, ws.data_ptr(), ws.numel(),
         _stream(p.device))
    return out, coeffs, al


def aligned_depth_metrics(pred, target, mask, align: str = "lstsq", clamp: bool = True, min_depth: float = 1e-3,
                          per_image: bool = False, return_coeffs: bool = False, return_aligned: bool = False):
    """The depth metrics of the prediction fitted to the target per image (align 'lstsq' or 'median'; with clamp the fitted
    value is clamped to [0, 1], paper_code/test_depth.py:207), keys ALIGNED_DEPTH_FIELDS, as fp64 CUDA tensors: 0-d for the
    whole batch (the reference's get_metrics on the stacked fitted batch) or [B] with per_image.  abs_rel .. delta3 are
    taken over the valid pixels with both depths floored at min_depth.  With return_coeffs / return_aligned the result is a
    tuple (dict, coeffs [B,2] fp32 = scale, shift, aligned [B,1,H,W] fp32), the absent ones left out.  No synchronisation."""
    rows, coeffs, al = _aligned_rows(pred, target, mask, align, clamp, min_depth, return_aligned)
    B = coeffs.shape[0]
    d = _as_dict(rows[:B] if per_image else rows[B:], ALIGNED_DEPTH_FIELDS, per_image)
    if not (return_coeffs or return_aligned):
        return d
    return (d,) + ((coeffs,) if return_coeffs else ()) + ((al,) if return_aligned else ())


def align_depth(pred, target, mask, align: str = "lstsq"):
    """-> (aligned [B,1,H,W] fp32, coeffs [B,2] fp32 = scale, shift): the prediction fitted to the target per image, not
    clamped, at every pixel (masked or not)."""
    _, coeffs, al = _aligned_rows(pred, target, mask, align, False, 1e-3, True)
    return al, coeffs


def get_metrics(pred, target, task=None, masks=None, align=None, clamp: bool = True, min_depth: float = 1e-3) -> Optional[Dict[str, float]]:
    """Reference-shaped entry point (:13): task in {'normal', 'depth_zbuffer'} -> dict of Python floats with the reference's
    keys, or None for an empty mask; one device-to-host copy of the row.  Any other task (the reference's task-less L1 / MSE
    included) raises ValueError.  With align ('lstsq' / 'median', depth only) the row is that of aligned_depth_metrics for
    the whole batch, with its seven further keys."""
    if align is not None:
        _check_align(task, align, min_depth)
        rows, _, _ = _aligned_rows(pred, target, masks, align, clamp, min_depth)
        row = rows[-1].cpu().tolist()
        return None if row[0] < 1.0 else dict(zip(ALIGNED_DEPTH_FIELDS[1:], row[1:]))
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
    the sums: sqrt(max(sumsq - sum^2 / n, 0) / (n - 1)); NaN for n < 2, and mean NaN for n == 0.

    With align ('lstsq' / 'median', task 'depth_zbuffer' only) the rows are the per-image rows of aligned_depth_metrics: every
    image fitted to its own ground truth, the keys ALIGNED_DEPTH_FIELDS."""

    def __init__(self, task: str, align=None, clamp: bool = True, min_depth: float = 1e-3):
        _, _, self.fields = _task(task)
        self.task = task
        self.align, self.clamp, self.min_depth = align, clamp, min_depth
        if align is not None:   # the per-image rows of aligned_depth_metrics
            _check_align(task, align, min_depth)
            self.fields = ALIGNED_DEPTH_FIELDS
        self._acc = None   # fp64 [3, fields]: count, sum, sum of squares

    def update(self, pred, target, mask) -> None:
        if self.align is not None:
            rows = _aligned_rows(pred, target, mask, self.align, self.clamp, self.min_depth)[0][:-1]
        else:
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
