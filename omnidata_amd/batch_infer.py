"""Image-set inference: a folder (or any sequence) of images of different sizes through the batched engine.

Per batch: decode in a thread pool -> one packed upload -> dptx_preprocess_u8_batch -> model(x) -> batched post-processing
-> one download into pinned memory -> PNG encode in the thread pool.  Batch k+1 is decoded while batch k is on the GPU and
batch k-1 is being encoded.  The files written are those of demo.py's per-image loop, pixel for pixel.

full_frame="squash" / "aspect" keeps the whole image instead of the centre crop and returns maps of the image's own size:
dptx_preprocess_u8_rect_batch -> model(x) at a rectangular network size -> dptx_postprocess_resize_batch.  "squash" is the
reference's fixed-input protocol (paper_code/oasis_eval_tta.py:324-339: image_size x image_size whatever the aspect);
"aspect" takes the network size per image from the reference's Resize.get_size (modules/midas/transforms.py:94-160), buckets
the images by network shape and runs the largest shape first, so the model plans its arena once.

tta=<preset> (surface normals only) runs the test-time augmentation of paper_code/oasis_eval_tta.py:440-534 instead
(omnidata_amd/tta.py: every image through the preset's views, merged per pixel): maps of the image's own size, files as in the
full-frame modes.  With task="depth" it needs tta_align="lstsq" (tta.DepthTTA: every view is fitted to a whole-image anchor
view by least squares before the merge) and writes <stem>_depth.png as RGBA at the image's own size.

tiled=True | {tile, scale, overlap, ...} runs tiled high-resolution inference instead (omnidata_amd/tiled.py: overlapping tiles of
the image at the chosen pixel scale, blended with feathered weights; depth tiles are first aligned to a whole-image anchor): maps
of the image's own size, files as in the full-frame modes.  It excludes full_frame and tta.

guided=True | {radius, sigma_space, sigma_range} (with full_frame) replaces the last step, the plain bilinear / bicubic resize
to the image's own size, by guided upsampling (pp.guided_outputs_gpu, dptx_postprocess_guided_batch): a joint bilateral filter
whose guides are already on the device -- the uploaded uint8 pixels at full resolution and the network input at the map's.  One
forward per image, edges where the image has them.  It excludes tta and tiled.
"""
from __future__ import annotations

import math
import os
import warnings
from concurrent.futures import ThreadPoolExecutor

import torch
from PIL import Image

from . import preprocess as pp

MAX_WORKERS = 16


def _decode(item):
    if isinstance(item, (str, os.PathLike)):
        img = Image.open(item)
        img.load()
        return img
    return item


def _size_of(item):
    """(w, h) of an input without decoding it: a path's header, a PIL image's size, an array's shape."""
    if isinstance(item, (str, os.PathLike)):
        with Image.open(item) as img:
            return img.size
    if isinstance(item, Image.Image):
        return item.size
    h, w = item.shape[:2]
    return int(w), int(h)


def plan_full_frame(sizes, mode: str, image_size: int = 384, batch_size: int = 32, multiple: int = 32):
    """sizes [(w, h)] in input order -> (chunks, capped): chunks = [((net_h, net_w), [input indices])], every chunk one network
    shape and at most batch_size images in input order, the shape with the largest net_h * net_w first (then by first
    appearance); capped = the indices whose network size pp.full_frame_net_size() had to cut back.  mode "squash": one shape,
    image_size x image_size."""
    if mode not in ("squash", "aspect"):
        raise ValueError('full_frame must be None, "squash" or "aspect"')
    buckets, capped = {}, []
    for i, (w, h) in enumerate(sizes):
        if mode == "squash":
            net = (image_size, image_size)
        else:
            nw, nh, cut = pp.full_frame_net_size(w, h, image_size, multiple)
            net = (nh, nw)
            if cut:
                capped.append(i)
        buckets.setdefault(net, []).append(i)
    order = sorted(buckets, key=lambda net: (-net[0] * net[1], buckets[net][0]))
    chunks = [(net, buckets[net][k:k + batch_size]) for net in order for k in range(0, len(buckets[net]), batch_size)]
    return chunks, capped


def lookahead(pool, items, chunks, stop_on_error: bool = False):
    """Yields (indices, decoded images, error) per chunk of `chunks` (lists of indices into items), in order: the decodes of the
    next chunk are queued before this one is handed out, so they run while the caller has the GPU work of this one in flight.
    A decode that raises propagates; with stop_on_error it ends the sequence instead: the images before it in its chunk are
    handed out together with the exception, and the decodes queued behind it are cancelled."""
    def submit(k):
        return [pool.submit(_decode, items[i]) for i in chunks[k]] if k < len(chunks) else []

    futures = submit(0)
    for k, idxs in enumerate(chunks):
        following = submit(k + 1)
        images, error = [], None
        for f in futures:
            try:
                images.append(f.result())
            except Exception as e:  # noqa: BLE001 -- re-raised by the caller once the earlier images are done
                if not stop_on_error:
                    raise
                error = e
                break
        if error is not None:
            for f in following:
                f.cancel()
        yield idxs, images, error
        if error is not None:
            return
        futures = following


class BatchPredictor:
    def __init__(self, model, task: str, batch_size: int = 32, workers: int = 8, image_size: int = 384, full_frame=None,
                 renormalize: bool = False, tta=None, tta_merger: str = "median", tta_options=None, tta_align=None, tiled=None,
                 guided=None):
        if task not in ("normal", "depth"):
            raise ValueError("task should be one of the following: normal, depth")
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        if full_frame not in (None, "squash", "aspect"):
            raise ValueError('full_frame must be None, "squash" or "aspect"')
        if renormalize and (full_frame is None or task != "normal"):
            raise ValueError("renormalize applies to full-frame surface normals only")
        if tta_align not in (None, "lstsq"):
            raise ValueError('tta_align must be None or "lstsq"')
        if tta_align is not None and (tta is None or task != "depth"):
            raise ValueError("tta_align applies to depth with tta only")
        if tta is not None and full_frame is not None:
            raise ValueError("tta excludes full_frame")
        if tta is not None and task == "depth" and tta_align is None:
            raise ValueError('tta for depth needs tta_align="lstsq": the views of a scale-and-shift-ambiguous map cannot be '
                             "merged without the alignment step")
        if tiled is False:
            tiled = None
        if tiled is not None and (tta is not None or full_frame is not None):
            raise ValueError("tiled excludes full_frame and tta")
        if tiled is not None and tiled is not True and not isinstance(tiled, dict):
            raise ValueError("tiled must be None, True or a dict of TiledNormals' / TiledDepth's options")
        if guided is False:
            guided = None
        if guided is not None and (full_frame is None or tta is not None or tiled is not None):
            raise ValueError("guided needs full_frame and excludes tta and tiled")
        # None: the plain resize; else the keyword arguments of pp.guided_outputs_gpu
        self.guided = None if guided is None else pp.guided_params({} if guided is True else guided)
        self.full_frame, self.renormalize = full_frame, bool(renormalize)
        self.capped = []   # full_frame="aspect": input indices of the last run whose network size was cut back to the supported range
        self.model, self.task, self.batch_size, self.image_size = model, task, int(batch_size), int(image_size)
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("BatchPredictor needs the model on an AMD GPU: the forward is implemented as HIP kernels only")
        self._runner = None   # the TTA or tiled object that takes the images instead of the batched paths below
        if tta is not None and task == "depth":   # tta_options: DepthTTA's multiple / max_side / chunk_images
            from .tta import DepthTTA
            self._runner = DepthTTA(model, tta, tta_merger, tta_align, batch_size=self.batch_size, **(tta_options or {}))
        elif tta is not None:   # tta_options: NormalsTTA's multiple / max_side / chunk_images / normalize_views
            from .tta import NormalsTTA
            self._runner = NormalsTTA(model, tta, tta_merger, batch_size=self.batch_size, **(tta_options or {}))
        elif tiled is not None:   # the tiled classes are called as the TTA ones are: chunk_images inputs -> maps at their own sizes
            from .tiled import TiledDepth, TiledNormals
            options = dict(batch_size=self.batch_size, **({} if tiled is True else tiled))
            self._runner = (TiledDepth if task == "depth" else TiledNormals)(model, **options)

    # ---- GPU side of one batch: decoded images -> final pixels, still on the device
    def _run(self, images) -> torch.Tensor:
        """normal: [B,S,S,3] uint8; depth: [B,512,512,4] uint8 (viridis RGBA), as demo.py saves them."""
        with torch.no_grad():
            x = pp.images_to_input_gpu(images, self.task, self.image_size, self.device)
            y = self.model(x).clamp(min=0, max=1)
            if self.task == "depth":
                return pp.depths_to_rgba_gpu(pp.depths_to_512_gpu(y))
            return pp.normals_to_u8_gpu(y)

    # ---- full frame: the whole image in, a map of the image's own size out
    def _run_full(self, images, net_hw):
        """-> list of device tensors, image i at its own size: normal [H,W,3] uint8, depth [H,W,4] uint8 (viridis RGBA)."""
        if self.guided is not None:
            return self._run_guided(images, net_hw)
        with torch.no_grad():
            x = pp.images_to_input_rect_gpu(images, self.task, net_hw, self.device)
            y = self.model(x).clamp(min=0, max=1)
            sizes = [_size_of(im)[::-1] for im in images]
            if self.task == "depth":
                return pp.resize_outputs_gpu(y, sizes, "depth_rgba")
            return pp.resize_outputs_gpu(y, sizes, "normal_u8", self.renormalize)

    def _run_guided(self, images, net_hw):
        """_run_full with guided upsampling as the last step: the guides are the uploaded pixels and the network input (in
        [0, 1]: the depth models take it normalised to [-1, 1])."""
        with torch.no_grad():
            x, pixels, descs = pp.images_to_input_rect_gpu(images, self.task, net_hw, self.device, return_pixels=True)
            y = self.model(x).clamp(min=0, max=1)
            guide_lo = x * 0.5 + 0.5 if self.task == "depth" else x
            sizes = [_size_of(im)[::-1] for im in images]
            mode = "depth_rgba" if self.task == "depth" else "normal_u8"
            return pp.guided_outputs_gpu(y, guide_lo, pixels, descs, sizes, mode, self.renormalize, **self.guided)

    def _chunks(self, items, pool):
        """Yields (input indices, decoded images, outputs, error) per chunk; the next chunk is decoded while this one is on the GPU.
        Centre crop: batch_size inputs in input order, outputs one tensor [B,...]; an unreadable file ends the sequence, the
        images before it in its chunk handed out with the exception (lookahead's stop_on_error).  Full frame: the chunks of
        plan_full_frame(), in the plan's order; tta and tiled: chunk_images inputs in input order (one upload and one merge or
        blend each); outputs a list of tensors, image i at its own size.  There the sizes come from the files' headers first and
        a decode error propagates: an unreadable file raises before anything has run."""
        crop = self._runner is None and self.full_frame is None
        if self._runner is None and not crop:
            sizes = list(pool.map(_size_of, items))
            plan, self.capped = plan_full_frame(sizes, self.full_frame, self.image_size, self.batch_size)
            if self.capped:
                warnings.warn(f"full_frame='aspect': the network size of {len(self.capped)} image(s) was cut back to a side of "
                              f"{pp.MAX_NET_SIDE} (BatchPredictor.capped lists them)", stacklevel=3)
        else:
            step = self.batch_size if crop else self._runner.chunk_images
            plan = [(None, list(range(i, min(i + step, len(items))))) for i in range(0, len(items), step)]
        for (net_hw, _), (idxs, images, error) in zip(plan, lookahead(pool, items, [idxs for _, idxs in plan], crop)):
            if crop:
                outs = self._run(images) if images else None
            else:
                outs = self._runner(images) if self._runner is not None else self._run_full(images, net_hw)
            yield idxs, images, outs, error

    def predict(self, images_or_paths):
        """Yields one device tensor per input, in input order (normal: [S,S,3] uint8, depth: [512,512,4] uint8 RGBA; with
        full_frame, tta or tiled the image's own size: [H,W,3] uint8, depth [H,W,4] uint8 RGBA).  Nothing is read back."""
        items = list(images_or_paths)
        ready, nxt = {}, 0   # outputs that wait for an earlier input of another bucket stay on the device
        with ThreadPoolExecutor(self.workers) as pool:
            for idxs, images, outs, error in self._chunks(items, pool):
                ready.update(zip(idxs, outs if images else ()))
                while nxt in ready:
                    yield ready.pop(nxt)
                    nxt += 1
                if error is not None:
                    raise error

    def predict_to_dir(self, paths, output_path, verbose: bool = False):
        """Writes <stem>_<task>.png and <stem>_rgb.png for every path, as demo.py does; with `verbose` also its two lines per
        file, in input order.  An unreadable file raises what Image.open raises, after every earlier file has been written.
        With full_frame, tta or tiled: <stem>_<task>.png at the image's own size, <stem>_rgb.png = the image unchanged, and an
        unreadable file raises before anything is written."""
        paths = [os.fspath(p) for p in paths]
        os.makedirs(output_path, exist_ok=True)
        crop = self.full_frame is None and self._runner is None

        def save(img, pixels, stem):
            if crop:
                rgb = pp.rgb_preview(img)
            else:
                rgb = img if img.mode in ("1", "L", "LA", "P", "RGB", "RGBA", "I", "I;16") else img.convert("RGB")
            rgb.save(os.path.join(output_path, f"{stem}_rgb.png"))
            Image.fromarray(pixels).save(os.path.join(output_path, f"{stem}_{self.task}.png"))

        writes, nxt = {}, 0   # input index -> (future, save_path)

        def flush(everything):
            nonlocal nxt
            while nxt in writes and (everything or writes[nxt][0].done()):
                f, save_path = writes.pop(nxt)
                f.result()
                if verbose:
                    print(f"Reading input {paths[nxt]} ...")
                    print(f"Writing output {save_path} ...")
                nxt += 1

        def write(pool, idxs, images, flat, shapes):
            """One read-back of a chunk's pixels (flat: one device tensor, image i its next prod(shapes[i]) elements) into pinned
            memory, and one save per image in the pool."""
            host = torch.empty(flat.shape, dtype=flat.dtype, pin_memory=True)
            host.copy_(flat, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            arr, at = host.numpy(), 0
            for i, img, shape in zip(idxs, images, shapes):
                stem = os.path.splitext(os.path.basename(paths[i]))[0]
                pixels = arr[at:at + math.prod(shape)].reshape(shape)
                at += pixels.size
                writes[i] = (pool.submit(save, img, pixels, stem), os.path.join(output_path, f"{stem}_{self.task}.png"))

        with ThreadPoolExecutor(self.workers) as pool:
            for idxs, images, outs, error in self._chunks(paths, pool):
                if images and crop:
                    write(pool, idxs, images, outs.reshape(-1), [tuple(outs.shape[1:])] * len(images))
                elif images:
                    write(pool, idxs, images, torch.cat([o.reshape(-1) for o in outs]), [tuple(o.shape) for o in outs])
                flush(error is not None)
                if error is not None:
                    if verbose:
                        print(f"Reading input {paths[idxs[len(images)]]} ...")
                    raise error
            flush(True)
