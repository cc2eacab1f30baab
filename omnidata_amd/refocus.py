"""3D refocus augmentation on the GPU: drop-in for omnidata_tools/torch/data/refocus_augmentation.py.

The depth-aware defocus blur of the Omnidata paper: the depth is banded at its n+1 quantiles, every quantile gets the
Gaussian blur radius of a thin lens focused at one of them, and every pixel blends the two blur levels around its depth.
compute_quantiles / refocus_image / RefocusImageAugmentation keep the reference's names and semantics (:82-88, :143-157,
:163-203); the work runs in libdptx's refocus.hip (include/dptx.h dptx_refocus_*).  CUDA tensors only: there is no CPU
path, as everywhere in omnidata_amd.
"""
from __future__ import annotations

import torch

from ._native import call, check_cuda, workspace
from .engine import _stream

EPS = 1e-4          # compute_quantiles' eps as the reference's only caller passes it (:188); the kernel applies it
MAX_M = 1 << 24     # largest blur filter the kernels define results for


def _workspace(B: int, C_: int, H: int, W: int, n: int, device) -> torch.Tensor:
    return workspace("dptx_refocus_workspace_bytes", device, (B, C_, H, W, n),
                     f"unsupported refocus shape B={B} C={C_} H={H} W={W} n_quantiles={n} "
                     "(1 <= H, W <= 8192, H*W <= 2^24, B, C, n >= 1)")


def _check_cuda(name: str, t: torch.Tensor, dim: int) -> torch.Tensor:
    check_cuda(name, t)
    if t.dim() != dim:
        raise ValueError(f"{name} must be {dim}-D, got shape {tuple(t.shape)}")
    return t.detach().float().contiguous()


def compute_quantiles(depth: torch.Tensor, n_quantiles: int, eps: float = EPS) -> torch.Tensor:
    """[B, n+1] fp32: torch.quantile(depth.reshape(B, -1), arange(n+1) / n, dim=1) with q_0 -= eps, q_n += eps, transposed
    (:82-88, :187-189); the values of CPU torch.quantile, computed on the GPU by exact selection."""
    if eps != EPS:
        raise ValueError(f"the device kernel applies eps = {EPS} (the reference's value), got {eps}")
    d = _check_cuda("depth", depth, 4)
    B, _, H, W = d.shape
    n = int(n_quantiles)
    ws = _workspace(B, 1, H, W, n, d.device)
    q = torch.empty(B, n + 1, dtype=torch.float32, device=d.device)
    call("dptx_refocus_quantiles", d.data_ptr(), B, H, W, n, q.data_ptr(), ws.data_ptr(), ws.numel(), _stream(d.device))
    return q


def _check_domain(depth: torch.Tensor, q: torch.Tensor, focus: torch.Tensor, aperture: torch.Tensor) -> None:
    """Raises ValueError where the reference raises: a NaN or +inf radius (int(nan) / int(inf) at :37; NaN / inf depth, a
    quantile of exactly 0), a filter wider than 2^24 taps, or a depth outside (q_0, q_n] (an out-of-range gather at
    :96-97).  One device->host read."""
    B = q.shape[0]
    r = aperture.reshape(B, 1) * torch.abs(q - focus.reshape(B, 1)) / q
    bad = torch.isnan(r) | ((r >= 0.1) & (r * 3 >= MAX_M))
    d = depth.reshape(B, -1)
    flags = torch.stack([bad.any(), ~torch.isfinite(d).all(), (d.amin(1) <= q[:, 0]).any(), (d.amax(1) > q[:, -1]).any()])
    f = flags.tolist()
    if f[1]:
        raise ValueError("refocus: depth has non-finite values (the reference's blur radii are then NaN)")
    if f[0]:
        raise ValueError("refocus: a blur radius is NaN / +inf or its filter exceeds 2^24 taps (the reference raises)")
    if f[2] or f[3]:
        raise ValueError("refocus: depth outside (q_0, q_n] (the reference's gather is out of range)")


def refocus_image(rgb: torch.Tensor, depth: torch.Tensor, focus_distance, aperture_size, quantile_vals: torch.Tensor,
                  return_segments: bool = False):
    """refocus_image (:143-157).  rgb [B,C,H,W], depth [B,1,H,W], focus_distance / aperture_size [B,1] or [B],
    quantile_vals [B, n+1] -> [B,C,H,W] (and the left segment index [B,1,H,W] int64 if return_segments)."""
    x = _check_cuda("rgb", rgb, 4)
    d = _check_cuda("depth", depth, 4)
    q = _check_cuda("quantile_vals", quantile_vals, 2)
    B, C_, H, W = x.shape
    if d.shape != (B, 1, H, W):
        raise ValueError(f"depth must be [B,1,H,W] = {(B, 1, H, W)}, got {tuple(d.shape)}")
    n = q.shape[1] - 1
    if q.shape[0] != B or n < 1:
        raise ValueError(f"quantile_vals must be [B, n+1] with n >= 1, got {tuple(q.shape)}")
    f = torch.as_tensor(focus_distance, dtype=torch.float32, device=x.device).reshape(-1).contiguous()
    a = torch.as_tensor(aperture_size, dtype=torch.float32, device=x.device).reshape(-1).contiguous()
    if f.numel() == 1 and B > 1:
        f = f.expand(B).contiguous()
    if a.numel() == 1 and B > 1:
        a = a.expand(B).contiguous()
    if f.numel() != B or a.numel() != B:
        raise ValueError("focus_distance and aperture_size need one value per image")
    ws = _workspace(B, C_, H, W, n, x.device)
    _check_domain(d, q, f, a)
    out = torch.empty_like(x)
    seg = torch.empty(B, 1, H, W, dtype=torch.int64, device=x.device) if return_segments else None
    call("dptx_refocus", x.data_ptr(), d.data_ptr(), B, C_, H, W, n, q.data_ptr(), f.data_ptr(), a.data_ptr(), out.data_ptr(),
         seg.data_ptr() if seg is not None else None, ws.data_ptr(), ws.numel(), _stream(x.device))
    return (out, seg) if return_segments else out


def draw(B: int, n_quantiles: int, aperture_min: float, aperture_max: float, device) -> tuple[torch.Tensor, torch.Tensor]:
    """The reference's random draws (:191-200), the same torch RNG calls in the same order on the same device: focus
    quantile index [B] int64 in [1, n), aperture [B, 1] log-uniform in [aperture_min, aperture_max]."""
    idx = torch.randint(low=1, high=n_quantiles, size=(B,), device=device)
    log_min = torch.log(torch.tensor(aperture_min, device=device))
    log_max = torch.log(torch.tensor(aperture_max, device=device))
    ap = torch.exp(torch.rand(size=(B, 1), device=device) * (log_max - log_min) + log_min)
    return idx, ap


def RefocusImageAugmentation(n_quantiles: int, aperture_min: float, aperture_max: float, return_segments: bool = False):
    """RefocusImageAugmentation (:163-203): returns f(rgb, depth) that refocuses every image at one of its quantiles
    (index drawn uniformly from [1, n)) with an aperture drawn log-uniformly from [aperture_min, aperture_max].  For a
    given torch seed the draws are those of the reference on the same device."""
    n = int(n_quantiles)

    def refocus_image_(rgb, depth):
        with torch.no_grad():
            q = compute_quantiles(depth, n, eps=EPS)
            idx, ap = draw(rgb.shape[0], n, aperture_min, aperture_max, depth.device)
            focus = torch.gather(q, 1, idx.unsqueeze(1))
            return refocus_image(rgb, depth, focus, ap, q, return_segments)

    return refocus_image_
