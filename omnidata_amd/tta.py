"""Test-time augmentation for surface normals: the benchmark protocol of the reference's paper_code/oasis_eval_tta.py.

oasis_eval_tta.py:440-448 wraps the model in SurfaceNormalsTTAWrapper(model_fn, transforms, run_mode='serial',
merger_fn=MedianMerger); lines 487-534 give the view sets: SurfaceNormalHorizontalFlip(dim_horizontal=0) x FiveCrops(0.8 | 0.9)
x ResizeShortestEdge([...]), chained to 40 views per image.  Every view goes through the network, is mapped back (un-mirrored
with the x component negated, resized into its crop window), the views that cover a pixel are merged by the per-channel median,
and the result is normalised again.  The wrapper's own package (`soda`) is not part of the reference tree, so nothing here could
be compared against it: the script pins the protocol, and this module fixes the details the script leaves open.

Definitions
  FiveCrops(f) on an H x W image: windows of ch = max(1, round(f * H)) rows and cw = max(1, round(f * W)) columns (Python's
    round) at top-left, top-right, bottom-left, bottom-right and centre, in that order; the centre window starts at
    ((H - ch) // 2, (W - cw) // 2).  f = 1.0 is the whole image, once.
  Network size of a window at short side s: preprocess.full_frame_net_size(cw, ch, s, multiple), cut back to max_side.
  View order: the preset's groups in order, then the crops in the order above, then the short sides as listed, the unflipped
    view before the flipped one.
  Merger: np.median -- the mean of the two middle values for an even count -- not torch's lower median: with the flip every
    count is even, and a lower median would be biased.  "mean" is the fp32 mean in view order.
  A view is decoded (2m - 1) and normalised at the network's resolution (oasis_eval_tta.py:441-445; the OASIS z-sign change of
    line 442 is not reproduced), resized with F.interpolate(mode='bilinear', align_corners=False); the merge is normalised again.

Depth is out of scope: crops of a scale-and-shift-ambiguous map cannot be merged without an alignment step.
"""
from __future__ import annotations

import torch
from PIL import Image

from . import preprocess as pp

# (fraction, short sides, flip) groups; oasis_eval_tta.py:487-534: small_crop_transforms, crop_transforms, whole_transforms
PRESETS = {
    "flip": [(1.0, [384], True)],
    "whole": [(1.0, [512, 256, 320, 384, 448], True)],
    "crops": [(0.9, [512, 256], True)],
    "oasis": [(0.8, [512], True), (0.9, [512, 256], True), (1.0, [512, 256, 320, 384, 448], True)],
}


def five_crops(w: int, h: int, fraction: float):
    """-> the windows (left, top, right, bottom) of FiveCrops(fraction) on a w x h image (see the module's definitions)."""
    if not 0 < fraction <= 1:
        raise ValueError("a crop fraction must be in (0, 1]")
    if fraction == 1:
        return [(0, 0, w, h)]
    ch, cw = max(1, round(fraction * h)), max(1, round(fraction * w))
    corners = [(0, 0), (w - cw, 0), (0, h - ch), (w - cw, h - ch), ((w - cw) // 2, (h - ch) // 2)]
    return [(x0, y0, x0 + cw, y0 + ch) for x0, y0 in corners]


def plan_views(w: int, h: int, preset="oasis", multiple: int = 32, max_side: int = 1024):
    """-> [(box, flip, short_side, (net_h, net_w))] for a w x h image, in view order: box = (left, top, right, bottom) as
    PIL's crop takes it.  preset: a name of PRESETS or a list of (fraction, short_sides, flip) groups."""
    groups = PRESETS.get(preset) if isinstance(preset, str) else list(preset)
    if groups is None:
        raise ValueError(f"tta preset must be one of {sorted(PRESETS)} or a list of (fraction, short_sides, flip)")
    top = max_side // multiple * multiple
    views = []
    for fraction, short_sides, flip in groups:
        for box in five_crops(w, h, fraction):
            for s in short_sides:
                nw, nh, _ = pp.full_frame_net_size(box[2] - box[0], box[3] - box[1], int(s), multiple)
                net = (min(nh, top), min(nw, top))
                views.append((box, False, int(s), net))
                if flip:
                    views.append((box, True, int(s), net))
    if not 1 <= len(views) <= pp.TTA_MAX_VIEWS:
        raise ValueError(f"a preset must give 1..{pp.TTA_MAX_VIEWS} views per image, not {len(views)}")
    return views


def _as_image(img):
    """What pack_images takes: RGB / L stay, every other PIL mode is converted to RGB."""
    if isinstance(img, Image.Image) and img.mode not in ("RGB", "L"):
        return img.convert("RGB")
    return img


class NormalsTTA:
    """model: a surface-normal network on the GPU, x [B,3,h,w] in [0, 1] -> [B,3,h,w] (encoded normals), for any h, w that are
    multiples of `multiple` up to `max_side` and B <= batch_size.  The version-1 UNet takes multiple=64, max_side=512."""

    def __init__(self, model, preset="oasis", merger: str = "median", normalize_views: bool = True, batch_size: int = 32,
                 multiple: int = 32, max_side: int = 1024, chunk_images: int = 8):
        if merger not in ("median", "mean"):
            raise ValueError('merger must be "median" or "mean"')
        if batch_size < 1 or chunk_images < 1:
            raise ValueError("batch_size and chunk_images must be >= 1")
        plan_views(64, 64, preset, multiple, max_side)   # an unknown preset raises here
        self.model, self.preset, self.merger, self.normalize_views = model, preset, merger, bool(normalize_views)
        self.batch_size, self.multiple, self.max_side, self.chunk_images = int(batch_size), int(multiple), int(max_side), int(chunk_images)
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("NormalsTTA needs the model on an AMD GPU: the forward and the merge are HIP kernels only")

    def _chunk(self, images, output):
        images = [_as_image(im) for im in images]
        buf, descs = pp.pack_images(images)                      # every image is uploaded once
        plans = [plan_views(d.W, d.H, self.preset, self.multiple, self.max_side) for d in descs[:len(images)]]
        flat = [(i, v) for i, plan in enumerate(plans) for v in plan]            # the merge's order: image-major
        buckets = {}
        for k, (_, (_, _, _, net)) in enumerate(flat):
            buckets.setdefault(net, []).append(k)
        order = sorted(buckets, key=lambda net: (-net[0] * net[1], buckets[net][0]))   # the largest shape first: one arena plan
        # the maps are stored bucket by bucket, so a forward's output is one contiguous copy
        at, total = {}, 0
        for net in order:
            for k in buckets[net]:
                at[k] = total
                total += 3 * net[0] * net[1]
        with torch.no_grad(), torch.cuda.device(self.device):
            dev = buf.to(self.device, non_blocking=True)
            maps = torch.empty(total, dtype=torch.float32, device=self.device)
            for net in order:
                ks = buckets[net]
                for b0 in range(0, len(ks), self.batch_size):
                    part = ks[b0:b0 + self.batch_size]
                    x = pp.views_to_input_gpu(dev, [pp.window_desc(descs[flat[k][0]], flat[k][1][0]) for k in part],
                                              [flat[k][1][1] for k in part], net, "normal")
                    n = len(part) * 3 * net[0] * net[1]
                    maps[at[part[0]]:at[part[0]] + n].view(len(part), 3, *net).copy_(self.model(x))
            views = [pp.TtaView(4 * at[k], net[0], net[1], i, box[1], box[0], box[3] - box[1], box[2] - box[0], int(flip))
                     for k, (i, (box, flip, _, net)) in enumerate(flat)]
            return pp.merge_normal_views_gpu(maps, views, [(d.H, d.W) for d in descs[:len(images)]], self.merger,
                                             self.normalize_views, output)

    def __call__(self, images, output: str = "u8"):
        """images: PIL images or uint8 HW[C] arrays -> list of device tensors at each image's own size: [H,W,3] uint8, or
        [3,H,W] fp32 with output="f32".  chunk_images images share one upload and one merge call."""
        if output not in ("u8", "f32"):
            raise ValueError('output must be "u8" or "f32"')
        images = list(images)
        res = []
        for c0 in range(0, len(images), self.chunk_images):
            res += self._chunk(images[c0:c0 + self.chunk_images], output)
        return res
