"""Tiled high-resolution inference: an image of any size up to 16384 a side is cut into overlapping windows of one size, every
window goes through the network at the chosen pixel scale, and the maps are blended into a map of the image's own size with a
feathered weight, so that no seam shows at a tile edge.  Every other inference path shows the network at most a 1024-pixel side
of the image and blows the map back up.  The reference has no tiled script: these definitions pin the protocol (include/dptx.h
states them for the C entry points, csrc/tiles.hip implements them).

Definitions
  Planner, plan_tiles(w, h, tile=384, scale=1.0, overlap=0.25, multiple=32, max_side=1024): T = int(tile * scale + 0.5); the
    window is cw = min(w, T), ch = min(h, T); every tile's network size is preprocess.full_frame_net_size(cw, ch, tile, multiple),
    cut back to max_side (a square window gives (tile, tile)).  Ramp per axis: r = min(int(overlap * c + 0.5), c // 2), with
    0 <= overlap <= 0.5.  Starts along an axis of length L: [0] where c == L; otherwise n = ceil((L - r) / (c - r)) windows at
    s_i = (i * (L - c) + (n - 1) // 2) // (n - 1): the first start is 0, the last window ends at L, and neighbouring windows
    overlap by at least r.  More than 64 starts on an axis raises ValueError.  Depth also plans one anchor: the whole image at
    preprocess.full_frame_net_size(w, h, 384, multiple), cut back to max_side.
  Tile value: the TTA merges' step for an unflipped view (omnidata_amd/tta.py).  Normals: n = 2m - 1, normalised at the network's
    resolution (normalize_views); depth: d = clamp(m, 0, 1).  Then F.interpolate(mode='bilinear', align_corners=False) into the
    window.
  Weight at local coordinate t in [0, c) of an axis with ramp r and start s, in fp32:
      left  = 1 if s == 0 or r == 0 else min(1, (t + 0.5) / r)
      right = 1 if s + c == L or r == 0 else min(1, ((c - 1 - t) + 0.5) / r)
    w_axis = left * right and w = w_y * w_x: an edge on the image border is not ramped, w > 0 everywhere in a window, and the sum
    of the weights is >= 1 wherever the grid covers.
  Blend: the tiles in grid order (iy ascending, then ix ascending), every step an fp32 multiply, then an add.  Normals:
    acc_c += w * v_c, then F.normalize (eps 1e-12) and (n + 1) / 2, clamped and quantised as resize_outputs_gpu does.  Depth:
    acc += w * (scale_k * r_k + shift_k) and wsum += w, then acc / wsum, clamp(0, 1) and 1 - x, the convention of
    resize_outputs_gpu(..., "depth_f32").  The anchor is used for the alignment only; it is not blended.
  Alignment (depth): every tile is fitted to its image's anchor by the least squares of DepthTTA (tta.py, "Alignment"),
    unchanged and by the same device code: a tile's coefficients equal, bit for bit, what align_depth_views_gpu gives for the same
    window and anchor.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import preprocess as pp
from .tta import _as_image, _Chunked, _forward_views, _require_depth_model

TilePlan = namedtuple("TilePlan", "net window ramps ys xs anchor_net")
TilePlan.__doc__ = """net (h, w): every tile's network size; window (ch, cw); ramps (ramp_y, ramp_x); ys / xs: the starts per axis;
anchor_net (ah, aw): the network size of the whole-image anchor that depth aligns its tiles to."""


def _starts(L: int, c: int, r: int):
    if c == L:
        return [0]
    n = -(-(L - r) // (c - r))
    return [(i * (L - c) + (n - 1) // 2) // (n - 1) for i in range(n)]


def plan_tiles(w: int, h: int, tile: int = 384, scale: float = 1.0, overlap: float = 0.25, multiple: int = 32, max_side: int = 1024):
    """-> TilePlan for a w x h image (the module's definitions).  tile: the network's short side for a tile; scale: image pixels
    per network pixel along a full tile's side (2.0 shows the network windows of twice the side); overlap: the ramp as a fraction
    of the window."""
    w, h, tile = int(w), int(h), int(tile)
    if w < 1 or h < 1 or tile < 1 or not scale > 0:
        raise ValueError("image sides, tile and scale must be positive")
    if not 0 <= overlap <= 0.5:
        raise ValueError("overlap must be in [0, 0.5]")
    T = int(tile * scale + 0.5)
    if T < 1:
        raise ValueError("tile * scale must give a window of at least one pixel")
    cw, ch = min(w, T), min(h, T)
    top = max_side // multiple * multiple
    nw, nh, _ = pp.full_frame_net_size(cw, ch, tile, multiple)
    ry, rx = min(int(overlap * ch + 0.5), ch // 2), min(int(overlap * cw + 0.5), cw // 2)
    ys, xs = _starts(h, ch, ry), _starts(w, cw, rx)
    if len(ys) > pp.TILE_MAX_AXIS or len(xs) > pp.TILE_MAX_AXIS:
        raise ValueError(f"{len(ys)} x {len(xs)} tiles: a grid has at most {pp.TILE_MAX_AXIS} per axis (take a larger tile or scale)")
    aw, ah, _ = pp.full_frame_net_size(w, h, 384, multiple)
    return TilePlan((min(nh, top), min(nw, top)), (ch, cw), (ry, rx), ys, xs, (min(ah, top), min(aw, top)))


def _tile_views(plan: TilePlan, tile: int):
    """The tiles of a plan as _forward_views takes views, in grid order."""
    (ch, cw) = plan.window
    return [((x0, y0, x0 + cw, y0 + ch), False, tile, plan.net) for y0 in plan.ys for x0 in plan.xs]


class _Tiled(_Chunked):
    channels, task, kernels = 3, "normal", "the forward and the blend"

    def __init__(self, model, tile, scale, overlap, batch_size, multiple, max_side, chunk_images):
        super().__init__(model, batch_size, multiple, max_side, chunk_images,   # a bad tile, scale or overlap raises here
                         lambda: plan_tiles(64, 64, tile, scale, overlap, multiple, max_side))
        self.tile, self.scale, self.overlap = int(tile), float(scale), float(overlap)

    def _forward(self, images, with_anchor: bool):
        """-> (maps, [TileGrid] per image, [(H, W)]): every tile (and with_anchor the whole image first) through the network."""
        planned = []

        def plans(descs):
            res = []
            for d in descs:
                p = plan_tiles(d.W, d.H, self.tile, self.scale, self.overlap, self.multiple, self.max_side)
                planned.append(p)
                anchor = [((0, 0, d.W, d.H), False, 384, p.anchor_net)] if with_anchor else []
                res.append(anchor + _tile_views(p, self.tile))
            return res

        maps, views, sizes = _forward_views(self.model, images, plans, self.batch_size, self.device, self.channels, self.task)
        grids, k = [], 0
        for p in planned:
            anchor_offset, anchor_hw = -1, (0, 0)
            if with_anchor:
                anchor_offset, anchor_hw = views[k].offset, p.anchor_net
                k += 1
            n, step = len(p.ys) * len(p.xs), 4 * self.channels * p.net[0] * p.net[1]
            # one network shape per image and _forward_views' bucket order: an image's tiles lie one behind the other
            assert all(views[k + j].offset == views[k].offset + j * step for j in range(n))
            grids.append(pp.TileGrid.make(views[k].offset, p.net, p.window, p.ys, p.xs, p.ramps, anchor_offset, anchor_hw))
            k += n
        return maps, grids, sizes


class TiledNormals(_Tiled):
    """model: a surface-normal network on the GPU, x [B,3,h,w] in [0, 1] -> [B,3,h,w] (encoded normals), for any h, w that are
    multiples of `multiple` up to `max_side` and B <= batch_size.  The version-1 UNet takes multiple=64, max_side=512.
    Called with images: [H,W,3] uint8 per image, or [3,H,W] fp32 with output="f32"; chunk_images images share one upload and one
    blend call."""

    def __init__(self, model, tile: int = 384, scale: float = 1.0, overlap: float = 0.25, normalize_views: bool = True,
                 batch_size: int = 32, multiple: int = 32, max_side: int = 1024, chunk_images: int = 1):
        super().__init__(model, tile, scale, overlap, batch_size, multiple, max_side, chunk_images)
        self.normalize_views = bool(normalize_views)

    def _chunk(self, images, output):
        images = [_as_image(im) for im in images]
        with torch.no_grad(), torch.cuda.device(self.device):
            maps, grids, sizes = self._forward(images, False)
            return pp.blend_normal_tiles_gpu(maps, grids, sizes, self.normalize_views, output)


class TiledDepth(_Tiled):
    """model: a DPT depth network (hybrid or large) on the GPU, x [B,3,h,w] in [-1, 1] -> [B,h,w].  align: "lstsq" fits every tile
    to the image's whole-image anchor before the blend (the module's definitions); None blends the tiles as they are, for
    comparison (no anchor is run then).
    Called with images: [H,W,4] uint8 per image (viridis over the map's own range), or [H,W] fp32 (1 - depth) with output="f32";
    the coefficients of return_coeffs are per tile, in grid order."""
    channels, task, outputs, aligned = 1, "depth", ("rgba", "f32"), True

    def __init__(self, model, tile: int = 384, scale: float = 1.0, overlap: float = 0.25, align="lstsq", batch_size: int = 32,
                 multiple: int = 32, max_side: int = 1024, chunk_images: int = 1):
        pp._one_of("align", align, ("lstsq", None))
        _require_depth_model(model, "TiledDepth")
        super().__init__(model, tile, scale, overlap, batch_size, multiple, max_side, chunk_images)
        self.align = align

    def _chunk(self, images, output, return_coeffs):
        images = [_as_image(im) for im in images]
        with torch.no_grad(), torch.cuda.device(self.device):
            maps, grids, sizes = self._forward(images, self.align is not None)
            coeffs = pp.align_depth_tiles_gpu(maps, grids, sizes) if self.align is not None else None
            res = pp.blend_depth_tiles_gpu(maps, grids, sizes, coeffs, output)
        if not return_coeffs:
            return res, None
        if coeffs is None:
            return res, [None] * len(images)
        return res, list(coeffs.split([g.tiles for g in grids]))
