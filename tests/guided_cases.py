"""The small cases the guided-upsampling tests share (tests/test_gpu_guided.py on the device, tests/test_guided_cpu_build.py on the
host build, tests/test_guided_host.py for the restatements alone), and the two restatements of every case, computed once.

A call shares the network shape h x w; its images have different sizes.  The shapes are the smallest at which the kernel can go
wrong: one row or column past a 64 x 8 tile (65 and 129 columns, 9 and 17 and 23 rows), h < 2R, more than one block, an output of
the map's own size, shrinking ones whose low-resolution footprint still fits the staging buffer (24x32 -> 13x11: 768 cells) and
ones where it does not (40x48 -> 13x11 and -> 8x64: 1920 cells, the taps come through the cache), a grey guide and a padded row
stride."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from guided_restatement import guided_values, finish

# name -> (h, w, [(H, W)], indices of grey guides, indices of guides with padded rows)
CALLS = {
    "5x7": (5, 7, [(23, 37), (9, 65), (5, 129)], (1,), (2,)),
    "3x2": (3, 2, [(9, 65), (23, 37), (3, 2)], (), (0,)),
    "4x4": (4, 4, [(5, 129), (4, 4), (17, 3)], (2,), ()),
    "24x32": (24, 32, [(13, 11), (23, 37), (24, 32)], (), (1,)),
    "40x48": (40, 48, [(13, 11), (8, 64), (50, 60)], (0,), ()),
    "6x6": (6, 6, [(6, 6)], (), ()),
}
RADII = (1, 2, 3)
SIGMA_RANGES = (0.05, 0.25)
SIGMA_SPACE = 1.0
PAD = 5   # bytes between the rows of a padded guide


@functools.lru_cache(maxsize=None)
def inputs(name, C):
    """-> (S [B,C,h,w] fp32, G_lo [B,3,h,w] fp32, [uint8 guide arrays [H,W] or [H,W,3]]): a random map, a random low-resolution
    colour field and, as the full-resolution guide, its bilinear resize with a little noise -- the two guides agree as an image and
    its network input do, so no tap wins by a margin that would hide the others."""
    h, w, outs, grey, _ = CALLS[name]
    g = torch.Generator().manual_seed(1000 * C + sum(map(ord, name)))
    B = len(outs)
    S = torch.rand(B, C, h, w, generator=g)
    G_lo = torch.rand(B, 3, h, w, generator=g)
    guides = []
    for i, (H, W) in enumerate(outs):
        if i in grey:
            G_lo[i] = G_lo[i, :1]
        hi = F.interpolate(G_lo[i:i + 1], size=(H, W), mode="bilinear", align_corners=False)[0]
        hi = (hi + 0.03 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
        u8 = (hi * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().numpy()
        guides.append(u8[:, :, 0].copy() if i in grey else u8)
    return S, G_lo, guides


@functools.lru_cache(maxsize=None)
def values(name, C, radius, sigma_range, dtype):
    """Steps 1-5 of every image of the call in `dtype`: a list of [C,H,W]."""
    S, G_lo, guides = inputs(name, C)
    return [guided_values(S[i], G_lo[i], guides[i], radius, SIGMA_SPACE, sigma_range, dtype) for i in range(len(guides))]


def restated(name, mode, renormalize, radius, sigma_range, dtype):
    """The call's outputs of 'normal_u8' / 'normal_f32' / 'depth_f32' in `dtype`."""
    return [finish(v, mode, renormalize) for v in values(name, 3 if mode.startswith("normal") else 1, radius, sigma_range, dtype)]


def pack_guides(name, guides):
    """-> (bytes [n] uint8, [(offset, H, W, C, row_stride_bytes)]): the guides back to back at odd offsets, the padded ones with
    PAD poisoned bytes between their rows, and not one byte behind the last pixel."""
    padded = CALLS[name][4]
    chunks, descs, off = [], [], 0
    for i, a in enumerate(guides):
        a = a[:, :, None] if a.ndim == 2 else a
        H, W, Cn = a.shape
        stride = W * Cn + (PAD if i in padded else 0)
        rows = np.full((H, stride), 0xEE, np.uint8)
        rows[:, :W * Cn] = a.reshape(H, W * Cn)
        flat = rows.reshape(-1)[:(H - 1) * stride + W * Cn]
        descs.append((off, H, W, Cn, stride))
        chunks.append(flat)
        off += flat.size
        if i + 1 < len(guides):
            chunks.append(np.full(3, 0xEE, np.uint8))   # the next image starts at an odd place
            off += 3
    return np.concatenate(chunks), descs
