"""Torch restatement of the reference's 3D refocus augmentation (omnidata_tools/torch/data/refocus_augmentation.py), the
yardstick of tests/test_refocus_host.py and tests/test_gpu_refocus.py.

Every discrete decision is taken in fp32 exactly as the reference takes it: the quantiles (CPU torch.quantile, :82-88),
the radii (:77-79), `r < 0.1` and M = int(3r) (+1 if even) (:34-38, :107-109), searchsorted (:93).  The blur itself is
fp64: the fp32 Gaussian taps of :16-29 are summed in fp64 into a dense [n, n] blur matrix per axis, with the replicate
padding of :51 folded in as clamped indices (the taps beyond |k| = n - 1 land on an edge for every pixel and are added
there as two tail sums).  No reference code is imported.
"""
from __future__ import annotations

import torch

QMAX_M = 1 << 24


def quantiles(depth: torch.Tensor, n: int, eps: float = 1e-4) -> torch.Tensor:
    """[B, n+1] fp32 on depth's device: CPU torch.quantile of the flattened depth, eps applied (:82-88, :187-189)."""
    B = depth.shape[0]
    q = torch.arange(0, n + 1) / n
    qv = torch.quantile(depth.detach().float().cpu().reshape(B, -1), q, dim=1)
    qv[0] -= eps
    qv[-1] += eps
    return qv.permute(1, 0).contiguous().to(depth.device)


def draw(B: int, n: int, aperture_min: float, aperture_max: float, device) -> tuple[torch.Tensor, torch.Tensor]:
    """The reference's random draws (:191-200), same calls in the same order: focus index [B] int64, aperture [B, 1]."""
    idx = torch.randint(low=1, high=n, size=(B,), device=device)
    log_min = torch.log(torch.tensor(aperture_min, device=device))
    log_max = torch.log(torch.tensor(aperture_max, device=device))
    ap = torch.exp(torch.rand(size=(B, 1), device=device) * (log_max - log_min) + log_min)
    return idx, ap


def radii(qvals: torch.Tensor, focus: torch.Tensor, aperture: torch.Tensor) -> torch.Tensor:
    """[B, n+1] fp32 (:77-79)."""
    B = qvals.shape[0]
    return aperture.float().reshape(B, 1) * torch.abs(qvals - focus.float().reshape(B, 1)) / qvals


def filter_size(r: torch.Tensor) -> int:
    """M of one level (:34-38 with cutoff int(3r), +1 if even, from :107-109); 1 = the level is the image itself."""
    if bool(r < 1e-1):
        return 1
    M = int(r * 3)
    if M % 2 == 0:
        M += 1
    return M


def blur_matrix(r: torch.Tensor, n: int) -> torch.Tensor:
    """[n, n] fp64: out = A @ x is one 1-D pass of separable_gaussian along an axis of length n (normalised by the fp64
    sum of the fp32 taps)."""
    M = filter_size(r)
    if M == 1:
        return torch.eye(n, dtype=torch.float64)
    if M > QMAX_M:
        raise ValueError(f"filter size {M} > 2^24")
    h = (M - 1) // 2
    k = torch.arange(0, h + 1, dtype=torch.float32)
    sig2 = 2 * r.float() * r.float()
    w = torch.exp(-k ** 2 / sig2).double()                          # taps 0..h (fp32, as gaussian() computes them)
    filsum = w[0] + 2 * w[1:].sum()
    inner = min(h, n - 1)
    offs = torch.arange(-inner, inner + 1)
    wk = w[offs.abs()]
    x = torch.arange(n)
    A = torch.zeros(n, n, dtype=torch.float64)
    A.scatter_add_(1, (x[:, None] + offs[None, :]).clamp(0, n - 1), wk[None, :].expand(n, -1).contiguous())
    tail = w[inner + 1:].sum()                                      # |k| > n-1: always beyond an edge
    A[:, 0] += tail
    A[:, n - 1] += tail
    return A / filsum


def refocus(rgb: torch.Tensor, depth: torch.Tensor, focus: torch.Tensor, aperture: torch.Tensor, qvals: torch.Tensor):
    """refocus_image (:143-157) -> (out [B,C,H,W] fp64 on CPU, segments [B,1,H,W] int64 on CPU)."""
    rgb = rgb.detach().double().cpu()
    depth = depth.detach().float().cpu()
    qvals = qvals.detach().float().cpu()
    B, C, H, W = rgb.shape
    n1 = qvals.shape[1]
    r = radii(qvals, focus.detach().cpu(), aperture.detach().cpu())
    d = depth.reshape(B, -1)
    right = torch.searchsorted(qvals, d)
    left = right - 1
    if int(left.min()) < 0 or int(right.max()) >= n1:
        raise ValueError("depth outside (q_0, q_n]")
    ql, qr = torch.gather(qvals, 1, left), torch.gather(qvals, 1, right)
    dist = qr - ql
    dl, dr = (d - ql) / dist, (qr - d) / dist
    sl, sr = 1 - dl ** 2, 1 - dr ** 2
    s = sl + sr
    wl, wr = (sl / s).double().reshape(B, 1, H, W), (sr / s).double().reshape(B, 1, H, W)
    out = torch.zeros(B, C, H, W, dtype=torch.float64)
    for b in range(B):
        used = set(left[b].unique().tolist()) | set(right[b].unique().tolist())
        for lv in sorted(used):
            Ah, Av = blur_matrix(r[b, lv], W), blur_matrix(r[b, lv], H)
            blurred = Av @ rgb[b] @ Ah.T
            m = (left[b] == lv).reshape(1, H, W).double() * wl[b] + (right[b] == lv).reshape(1, H, W).double() * wr[b]
            out[b] += m * blurred
    return out, left.reshape(B, 1, H, W)


def augment(rgb: torch.Tensor, depth: torch.Tensor, n: int, aperture_min: float, aperture_max: float):
    """RefocusImageAugmentation (:163-203): quantiles, then the draws on depth's device -> (out, segments, focus, aperture)."""
    qv = quantiles(depth, n)
    idx, ap = draw(rgb.shape[0], n, aperture_min, aperture_max, depth.device)
    focus = torch.gather(qv, 1, idx.unsqueeze(1))
    out, seg = refocus(rgb, depth, focus, ap, qv)
    return out, seg, focus, ap
