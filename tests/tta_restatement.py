"""The merge of test-time augmentation for surface normals (include/dptx.h dptx_tta_merge_normals, omnidata_amd/tta.py), restated
literally in torch and numpy: every view decoded, normalised at its own resolution, F.interpolate'd into its window of a
NaN-padded [views, 3, H, W] stack (a flipped view un-mirrored, x negated), np.nanmedian / np.nanmean over the views, normalised
and encoded.  dtype torch.float32 is the composition a user would write; torch.float64 is the reference the tests measure
against.  Also the synthetic views the GPU tests and the parity record use."""
import math
import warnings

import numpy as np
import torch
import torch.nn.functional as F


def merge_restatement(maps, views, size, merger="median", normalize_views=True, dtype=torch.float32, details=False):
    """maps: list of [3,h,w] fp32 tensors (encoded normals m); views: list of (y0, x0, ch, cw, flip); size (H, W) -> [3,H,W]
    encoded result in `dtype`.  details=True: also the shortest decoded view vector and the shortest merged vector (over the
    covered pixels), the quantities the final normalisations divide by."""
    H, W = size
    stack = torch.full((len(maps), 3, H, W), float("nan"), dtype=dtype)
    shortest_view = math.inf
    for k, (m, (y0, x0, ch, cw, flip)) in enumerate(zip(maps, views)):
        n = 2 * m.to(dtype) - 1
        shortest_view = min(shortest_view, float(n.norm(dim=0).min()))
        if normalize_views:
            n = F.normalize(n, p=2, dim=0, eps=1e-12)
        r = F.interpolate(n[None], (ch, cw), mode="bilinear", align_corners=False)[0]
        if flip:
            r = r.flip(-1)
            r[0] = -r[0]
        stack[k, :, y0:y0 + ch, x0:x0 + cw] = r
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # all-NaN slice: a pixel no view covers
        merged = (np.nanmedian if merger == "median" else np.nanmean)(stack.numpy(), axis=0)
    covered = ~np.isnan(merged[0])
    merged = torch.from_numpy(np.nan_to_num(merged, nan=0.0)).to(dtype)
    out = ((F.normalize(merged, p=2, dim=0, eps=1e-12) + 1) / 2).clamp(0, 1)
    if details:
        lengths = merged.norm(dim=0)[torch.from_numpy(covered)]
        return out, shortest_view, float(lengths.min()) if lengths.numel() else math.inf
    return out


def synthetic_view(k, h, w, window, size, noise=0.1):
    """View k's map [3,h,w] fp32: a smooth unit-normal field over the IMAGE, sampled where the view's pixels lie (mirrored, x
    negated for a flipped view: what a network that saw the mirrored window would return), times a random length in
    [0.7, 1.0] per pixel, plus Gaussian noise of `noise` per component; encoded (n + 1) / 2.  Seeded by k."""
    y0, x0, ch, cw, flip = window
    H, W = size
    g = torch.Generator().manual_seed(1000 + k)
    ys = y0 + (torch.arange(h, dtype=torch.float64) + 0.5) * ch / h
    xs = x0 + (torch.arange(w, dtype=torch.float64) + 0.5) * cw / w
    if flip:
        xs = x0 + cw - (torch.arange(w, dtype=torch.float64) + 0.5) * cw / w
    Y, X = torch.meshgrid(ys / H, xs / W, indexing="ij")
    n = torch.stack([0.6 * torch.sin(4.0 * X + 1.0 * Y), 0.6 * torch.cos(3.0 * Y - 2.0 * X), torch.ones_like(X)])
    n = n / n.norm(dim=0, keepdim=True)
    if flip:
        n[0] = -n[0]
    n = n * (0.7 + 0.3 * torch.rand(h, w, generator=g, dtype=torch.float64))
    n = n + noise * torch.randn(3, h, w, generator=g, dtype=torch.float64)
    return ((n + 1) / 2).float()
