"""Test-time augmentation for depth (include/dptx.h dptx_tta_align_depth / dptx_tta_merge_depth, omnidata_amd/tta.py), restated
literally in torch and numpy: every view clamped at its own resolution and F.interpolate'd into its window of a NaN-padded
[views, H, W] stack (a flipped view un-mirrored), the four sums of every view against the anchor over its window, the 2 x 2 solve,
scale * r + shift, np.nanmedian / np.nanmean over the views, clamp, 1 - x.  dtype torch.float32 is the composition a user would
write (sums and solve in fp32 too); torch.float64 is the reference the tests measure against.  Also the synthetic views -- one
smooth truth over the image, seen by every view through a planted affine map of its own -- that the tests share."""
import functools
import warnings

import numpy as np
import torch
import torch.nn.functional as F

DEGENERATE = 1e-10            # a view with det <= DEGENERATE * n * sum r^2 gets scale 1 and the mean difference as its shift


def align_merge_restatement(maps, views, size, anchor, merger="median", dtype=torch.float32, align=True, details=False):
    """maps: list of [h,w] fp32 tensors; views: list of (y0, x0, ch, cw, flip); size (H, W); anchor: index of the view that covers
    the image (ignored with align=False) -> (out [H,W] in `dtype`: 1 - merged depth, coeffs [views, 2] in `dtype`: scale, shift --
    (1, 0) rows with align=False).  details=True: also the smallest det / (n sum r^2) over the fitted views."""
    H, W = size
    stack = torch.full((len(maps), H, W), float("nan"), dtype=dtype)
    for k, (m, (y0, x0, ch, cw, flip)) in enumerate(zip(maps, views)):
        d = m.to(dtype).reshape(1, 1, *m.shape[-2:]).clamp(0, 1)
        r = F.interpolate(d, (ch, cw), mode="bilinear", align_corners=False)[0, 0]
        stack[k, y0:y0 + ch, x0:x0 + cw] = r.flip(-1) if flip else r
    coeffs = torch.zeros(len(maps), 2, dtype=dtype)
    coeffs[:, 0] = 1
    flattest = float("inf")
    if align:
        y0, x0, ch, cw, _ = views[anchor]
        assert (y0, x0, ch, cw) == (0, 0, H, W), "the anchor covers the whole image"
        for k, (y0, x0, ch, cw, _) in enumerate(views):
            if k == anchor:
                continue
            r = stack[k, y0:y0 + ch, x0:x0 + cw]
            a = stack[anchor, y0:y0 + ch, x0:x0 + cw]
            n = torch.tensor(float(ch * cw), dtype=dtype)
            sr, srr, sa, sra = r.sum(), (r * r).sum(), a.sum(), (r * a).sum()
            det = n * srr - sr * sr
            flattest = min(flattest, float(det / (n * srr)) if float(srr) > 0 else 0.0)
            if bool(det > DEGENERATE * n * srr):
                coeffs[k, 0] = (n * sra - sr * sa) / det
                coeffs[k, 1] = (srr * sa - sr * sra) / det
            else:
                coeffs[k, 1] = (sa - sr) / n
        stack = coeffs[:, 0, None, None] * stack + coeffs[:, 1, None, None]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # all-NaN slice: a pixel no view covers
        merged = (np.nanmedian if merger == "median" else np.nanmean)(stack.numpy(), axis=0)
    merged = torch.from_numpy(np.nan_to_num(merged, nan=0.0)).to(dtype)
    out = 1 - merged.clamp(0, 1)
    return (out, coeffs, flattest) if details else (out, coeffs)


def synthetic_depth_truth(ys, xs, size):
    """0.5 + 0.2 sin(4X + Y) cos(3Y - 2X) at image rows ys and columns xs (pixel units, centres at k + 0.5), X = x / W, Y = y / H."""
    H, W = size
    Y, X = torch.meshgrid(ys / H, xs / W, indexing="ij")
    return 0.5 + 0.2 * torch.sin(4.0 * X + 1.0 * Y) * torch.cos(3.0 * Y - 2.0 * X)


def image_truth(size):
    """The truth at the image's own pixel centres, [H,W] fp64: what a perfect merge returns (before the 1 - x)."""
    H, W = size
    return synthetic_depth_truth(torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5, size)


def _draw(k, anchor):
    g = torch.Generator().manual_seed(2000 + k)
    a, b = (float(v) for v in torch.rand(2, generator=g, dtype=torch.float64))
    return g, ((1.0, 0.0) if anchor else (0.8 + 0.45 * a, -0.05 + 0.1 * b))


def planted_coeffs(k, anchor=False):
    """(a, b) of view k: a in [0.8, 1.25], b in [-0.05, 0.05], seeded 2000 + k; the anchor has (1, 0)."""
    return _draw(k, anchor)[1]


def synthetic_depth_view(k, h, w, window, size, noise=0.01, anchor=False):
    """View k's map [h,w] fp32: the truth sampled at the centres of the view's pixels (mirrored for a flipped view), seen through
    the planted map -- (truth - b) / a, so that a * map + b is the truth -- plus Gaussian noise of `noise`.  Seeded by k."""
    y0, x0, ch, cw, flip = window
    g, (a, b) = _draw(k, anchor)
    ys = y0 + (torch.arange(h, dtype=torch.float64) + 0.5) * ch / h
    xs = x0 + (torch.arange(w, dtype=torch.float64) + 0.5) * cw / w
    if flip:
        xs = x0 + cw - (torch.arange(w, dtype=torch.float64) + 0.5) * cw / w
    m = (synthetic_depth_truth(ys, xs, size) - b) / a + noise * torch.randn(h, w, generator=g, dtype=torch.float64)
    return m.float()


# ------------------------------------------------------------------------------------------------ the cases the tests share
SIZE, EDGE = (70, 93), (9, 13)                                        # (H, W)
SCALED_OASIS = [(0.8, [192], True), (0.9, [192, 64], True), (1.0, [192, 64, 96, 128, 160], True)]   # "oasis" at 3/8 of its sides


def windows_of(plan):
    return [(box[1], box[0], box[3] - box[1], box[2] - box[0], int(flip)) for box, flip, _, _ in plan]


@functools.lru_cache(maxsize=None)
def oasis_depth_case():
    """-> (maps, windows, anchor): the 40 views of the scaled OASIS plan on a 70 x 93 image; the anchor is view 30."""
    from omnidata_amd.tta import plan_depth_views
    plan, anchor = plan_depth_views(SIZE[1], SIZE[0], SCALED_OASIS)
    assert len(plan) == 40 and anchor == 30
    windows = windows_of(plan)
    return tuple(synthetic_depth_view(k, *plan[k][3], windows[k], SIZE, anchor=k == anchor) for k in range(40)), tuple(windows), anchor


@functools.lru_cache(maxsize=None)
def oasis_depth_reference(merger, align=True):
    """-> (fp64 out, fp64 coeffs, e_ref, e_ref_c, smallest det / (n sum r^2)): e_ref / e_ref_c = the fp32 restatement's own distance
    from the fp64 one, output and coefficients."""
    maps, windows, anchor = oasis_depth_case()
    o64, c64, flattest = align_merge_restatement(maps, windows, SIZE, anchor, merger, torch.float64, align, details=True)
    o32, c32 = align_merge_restatement(maps, windows, SIZE, anchor, merger, torch.float32, align)
    return o64, c64, float((o32.double() - o64).abs().max()), float((c32.double() - c64).abs().max()), flattest


@functools.lru_cache(maxsize=None)
def stacked_depth_case(n):
    """n views of the whole 9 x 13 image (every pixel is covered n times), alternately plain and flipped, maps of 16 x 24; view 0
    is the anchor.  -> (maps, windows, 0)"""
    windows = tuple((0, 0, *EDGE, k % 2) for k in range(n))
    return tuple(synthetic_depth_view(100 + k, 16, 24, windows[k], EDGE, noise=0.03, anchor=k == 0) for k in range(n)), windows, 0


@functools.lru_cache(maxsize=None)
def stacked_depth_reference(n, merger):
    maps, windows, anchor = stacked_depth_case(n)
    o64, c64 = align_merge_restatement(maps, windows, EDGE, anchor, merger, torch.float64)
    o32, c32 = align_merge_restatement(maps, windows, EDGE, anchor, merger, torch.float32)
    return o64, c64, float((o32.double() - o64).abs().max()), float((c32.double() - c64).abs().max())
