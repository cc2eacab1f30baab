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

Depth (DepthTTA; the reference has no depth TTA script, so these definitions pin the protocol -- include/dptx.h states them
for the C entry points).  The network's depth is defined up to a scale and a shift per forward, and it is trained with the
least-squares alignment of losses/midas_loss.py:10-30 (compute_scale_and_shift): that alignment is the model's own notion of
"equal up to an affine map", and it is the step that makes crops mergeable.
  View value: d = clamp(m, 0, 1) at the network's resolution (demo.py:140), resized into its window with
    F.interpolate(mode='bilinear', align_corners=False); a flipped view is un-mirrored, no sign changes.  Coordinates and blend
    order are those of the normals merge.
  Anchor: one view per image that covers the whole image; its coefficients are exactly (1, 0).  DepthTTA takes the first
    unflipped whole-image view of the plan; a plan without one ("crops") gets ((0, 0, w, h), False, 384, net) prepended, and a
    plan that would then exceed 64 views raises.
  Alignment of a view k that is not the anchor: over all n = ch * cw pixels of its window, with r the view's value and a the
    anchor's value at the same image pixel (fp32 both), fp64 sums in a fixed order Sr, Srr, Sa, Sra; det = n Srr - Sr^2;
    scale = (n Sra - Sr Sa) / det, shift = (Srr Sa - Sr Sra) / det, solved in fp64 and rounded once to fp32.  A degenerate view,
    not (det > 1e-10 n Srr) -- flatter than 1e-5 of its own level --, gets scale = 1 and shift = (Sa - Sr) / n.  The solved scale
    is not clamped.
  Merge: the candidates scale_k * r_k + shift_k (an fp32 multiply, then an add) of the covering views in view order; np.median
    or the fp32 mean in view order; then clamp(0, 1) and 1 - x, the convention of resize_outputs_gpu(..., "depth_f32").
  Inputs are assumed finite; non-finite ones neither fault nor hang and affect only the image they belong to.
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


def plan_depth_views(w: int, h: int, preset="whole", multiple: int = 32, max_side: int = 1024):
    """-> (plan_views(...) with an anchor in it, the anchor's index): the anchor is the first unflipped view of the whole image;
    a plan without one gets ((0, 0, w, h), False, 384, net) prepended.  More than 64 views then raises."""
    views = plan_views(w, h, preset, multiple, max_side)
    for k, (box, flip, _, _) in enumerate(views):
        if box == (0, 0, w, h) and not flip:
            return views, k
    if len(views) + 1 > pp.TTA_MAX_VIEWS:
        raise ValueError(f"the preset gives {len(views)} views and none of the whole image: with the anchor that is more than "
                         f"{pp.TTA_MAX_VIEWS} per image")
    top = max_side // multiple * multiple
    nw, nh, _ = pp.full_frame_net_size(w, h, 384, multiple)
    return [((0, 0, w, h), False, 384, (min(nh, top), min(nw, top)))] + views, 0


def _forward_views(model, images, plans, batch_size: int, device, channels: int, task: str):
    """What NormalsTTA and DepthTTA share: the images uploaded once, every view of plans(descs)[i] (plan_views' tuples per
    image, from the images' descriptors) through the network -- bucketed by network shape, the largest shape first, batch_size views per forward -- and the maps laid
    out for the merge.  -> (maps: one fp32 device tensor, [TtaView] in the merge's image-major order with offsets into maps,
    [(H, W)] per image).  channels: of the network's map per view; task: what views_to_input_gpu normalises for."""
    buf, descs = pp.pack_images(images)                      # every image is uploaded once
    flat = [(i, v) for i, plan in enumerate(plans(descs[:len(images)])) for v in plan]   # the merge's order: image-major
    buckets = {}
    for k, (_, (_, _, _, net)) in enumerate(flat):
        buckets.setdefault(net, []).append(k)
    order = sorted(buckets, key=lambda net: (-net[0] * net[1], buckets[net][0]))   # the largest shape first: one arena plan
    # the maps are stored bucket by bucket, so a forward's output is one contiguous copy
    at, total = {}, 0
    for net in order:
        for k in buckets[net]:
            at[k] = total
            total += channels * net[0] * net[1]
    dev = buf.to(device, non_blocking=True)
    maps = torch.empty(total, dtype=torch.float32, device=device)
    for net in order:
        ks = buckets[net]
        for b0 in range(0, len(ks), batch_size):
            part = ks[b0:b0 + batch_size]
            x = pp.views_to_input_gpu(dev, [pp.window_desc(descs[flat[k][0]], flat[k][1][0]) for k in part],
                                      [flat[k][1][1] for k in part], net, task)
            n = len(part) * channels * net[0] * net[1]
            maps[at[part[0]]:at[part[0]] + n].view(len(part), channels, *net).copy_(model(x).reshape(len(part), channels, *net))
    views = [pp.TtaView(4 * at[k], net[0], net[1], i, box[1], box[0], box[3] - box[1], box[2] - box[0], int(flip))
             for k, (i, (box, flip, _, net)) in enumerate(flat)]
    return maps, views, [(d.H, d.W) for d in descs[:len(images)]]


def _require_depth_model(model, who: str) -> None:
    from .model import DPTDepthModel
    if not isinstance(model, DPTDepthModel) or model.num_channels != 1:
        raise ValueError(f"{who} takes a DPT depth model (build_model('depth', ...), hybrid or large)")


class _Chunked:
    """What NormalsTTA, DepthTTA and the classes of tiled.py share: the constructor's checks, and the call.

    obj(images, output=None, return_coeffs=False): images: PIL images or uint8 HW[C] arrays -> list of device tensors at each
    image's own size, in the form `output` names (None: the first of the class's `outputs`).  chunk_images images share one upload
    and one _chunk() call.  return_coeffs=True (the depth classes): -> (that list, per image the [n, 2] fp32 (scale, shift) of its
    views or tiles; None per image with align=None)."""
    outputs = ("u8", "f32")
    aligned = False                              # whether _chunk takes return_coeffs and returns (maps, coefficients)
    kernels = "the forward and the merge"

    def __init__(self, model, batch_size, multiple, max_side, chunk_images, check_plan):
        if batch_size < 1 or chunk_images < 1:
            raise ValueError("batch_size and chunk_images must be >= 1")
        check_plan()                             # the subclass's other rules: all decided before the model is touched
        self.model = model
        self.batch_size, self.multiple, self.max_side, self.chunk_images = int(batch_size), int(multiple), int(max_side), int(chunk_images)
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} needs the model on an AMD GPU: {self.kernels} are HIP kernels only")

    def __call__(self, images, output=None, return_coeffs: bool = False):
        output = self.outputs[0] if output is None else output
        pp._one_of("output", output, self.outputs)
        if return_coeffs and not self.aligned:
            raise TypeError(f"{type(self).__name__} has no coefficients to return")
        images = list(images)
        res, coeffs = [], []
        for c0 in range(0, len(images), self.chunk_images):
            r = self._chunk(images[c0:c0 + self.chunk_images], output, *((return_coeffs,) if self.aligned else ()))
            if self.aligned:
                r, c = r
                coeffs += c or []
            res += r
        return (res, coeffs) if return_coeffs else res


class NormalsTTA(_Chunked):
    """model: a surface-normal network on the GPU, x [B,3,h,w] in [0, 1] -> [B,3,h,w] (encoded normals), for any h, w that are
    multiples of `multiple` up to `max_side` and B <= batch_size.  The version-1 UNet takes multiple=64, max_side=512.
    Called with images: [H,W,3] uint8 per image, or [3,H,W] fp32 with output="f32"; chunk_images images share one upload and one
    merge call."""

    def __init__(self, model, preset="oasis", merger: str = "median", normalize_views: bool = True, batch_size: int = 32,
                 multiple: int = 32, max_side: int = 1024, chunk_images: int = 8):
        pp._one_of("merger", merger, ("median", "mean"))
        super().__init__(model, batch_size, multiple, max_side, chunk_images,
                         lambda: plan_views(64, 64, preset, multiple, max_side))   # an unknown preset raises here
        self.preset, self.merger, self.normalize_views = preset, merger, bool(normalize_views)

    def _chunk(self, images, output):
        images = [_as_image(im) for im in images]
        plans = lambda descs: [plan_views(d.W, d.H, self.preset, self.multiple, self.max_side) for d in descs]
        with torch.no_grad(), torch.cuda.device(self.device):
            maps, views, sizes = _forward_views(self.model, images, plans, self.batch_size, self.device, 3, "normal")
            return pp.merge_normal_views_gpu(maps, views, sizes, self.merger, self.normalize_views, output)


class DepthTTA(_Chunked):
    """model: a DPT depth network (hybrid or large) on the GPU, x [B,3,h,w] in [-1, 1] -> [B,h,w], for any h, w that are
    multiples of `multiple` up to `max_side` and B <= batch_size.  align: "lstsq" fits every view to the image's anchor view
    before the merge (the module's definitions); None merges the views as they are, for comparison.
    Called with images: [H,W,4] uint8 per image (viridis over the map's own range), or [H,W] fp32 (1 - depth, as
    resize_outputs_gpu(..., "depth_f32")) with output="f32"; the coefficients of return_coeffs are in plan_depth_views' order.
    chunk_images images share one upload, one alignment and one merge call."""
    outputs, aligned, kernels = ("rgba", "f32"), True, "the forward, the alignment and the merge"

    def __init__(self, model, preset="whole", merger: str = "median", align="lstsq", batch_size: int = 32, multiple: int = 32,
                 max_side: int = 1024, chunk_images: int = 8):
        def check_plan():
            _require_depth_model(model, "DepthTTA")
            plan_depth_views(64, 64, preset, multiple, max_side)   # an unknown preset raises here

        pp._one_of("merger", merger, ("median", "mean"))
        pp._one_of("align", align, ("lstsq", None))
        super().__init__(model, batch_size, multiple, max_side, chunk_images, check_plan)
        self.preset, self.merger, self.align = preset, merger, align

    def _chunk(self, images, output, return_coeffs):
        images = [_as_image(im) for im in images]
        anchors = []

        def plans(descs):
            planned = [plan_depth_views(d.W, d.H, self.preset, self.multiple, self.max_side) for d in descs]
            first = 0
            for plan, anchor in planned:
                anchors.append(first + anchor)
                first += len(plan)
            return [plan for plan, _ in planned]

        with torch.no_grad(), torch.cuda.device(self.device):
            maps, views, sizes = _forward_views(self.model, images, plans, self.batch_size, self.device, 1, "depth")
            coeffs = ws = None
            if self.align is not None:
                coeffs, ws = pp.align_depth_views_gpu(maps, views, anchors, sizes)
            res = pp.merge_depth_views_gpu(maps, views, sizes, coeffs, ws, self.merger, output)
        if not return_coeffs:
            return res, None
        if coeffs is None:
            return res, [None] * len(images)
        counts = [sum(1 for v in views if v.image == i) for i in range(len(images))]
        return res, list(coeffs.split(counts))
