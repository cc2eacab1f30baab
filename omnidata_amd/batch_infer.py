"""Image-set inference: a folder (or any sequence) of images of different sizes through the batched engine.

Per batch: decode in a thread pool -> one packed upload -> dptx_preprocess_u8_batch -> model(x) -> batched post-processing
-> one download into pinned memory -> PNG encode in the thread pool.  Batch k+1 is decoded while batch k is on the GPU and
batch k-1 is being encoded.  The files written are those of demo.py's per-image loop, pixel for pixel.
"""
from __future__ import annotations

import os
from collections import deque
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


class BatchPredictor:
    def __init__(self, model, task: str, batch_size: int = 32, workers: int = 8, image_size: int = 384):
        if task not in ("normal", "depth"):
            raise ValueError("task should be one of the following: normal, depth")
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.model, self.task, self.batch_size, self.image_size = model, task, int(batch_size), int(image_size)
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("BatchPredictor needs the model on an AMD GPU: the forward is implemented as HIP kernels only")

    # ---- GPU side of one batch: decoded images -> final pixels, still on the device
    def _run(self, images) -> torch.Tensor:
        """normal: [B,S,S,3] uint8; depth: [B,512,512,4] uint8 (viridis RGBA), as demo.py saves them."""
        with torch.no_grad():
            x = pp.images_to_input_gpu(images, self.task, self.image_size, self.device)
            y = self.model(x).clamp(min=0, max=1)
            if self.task == "depth":
                return pp.depths_to_rgba_gpu(pp.depths_to_512_gpu(y))
            return pp.normals_to_u8_gpu(y)

    def _batches(self, items, pool):
        """Yields (first index, decoded images, error): the decodes of the next batch are queued before this one is handed
        out, so they run while the caller has the GPU work of this one in flight.  A decode that raises ends the sequence:
        the images before it in its batch are handed out with the exception."""
        chunks = [items[i:i + self.batch_size] for i in range(0, len(items), self.batch_size)]
        if not chunks:
            return
        futures = [pool.submit(_decode, it) for it in chunks[0]]
        for k, _ in enumerate(chunks):
            nxt = [pool.submit(_decode, it) for it in chunks[k + 1]] if k + 1 < len(chunks) else []
            images, error = [], None
            for f in futures:
                try:
                    images.append(f.result())
                except Exception as e:  # noqa: BLE001 -- re-raised by the caller once the earlier images are done
                    error = e
                    break
            if error is not None:
                for f in nxt:
                    f.cancel()
            yield k * self.batch_size, images, error
            if error is not None:
                return
            futures = nxt

    def predict(self, images_or_paths):
        """Yields one device tensor per input, in input order (normal: [S,S,3] uint8, depth: [512,512,4] uint8 RGBA).
        Nothing is read back."""
        items = list(images_or_paths)
        with ThreadPoolExecutor(self.workers) as pool:
            for _, images, error in self._batches(items, pool):
                if images:
                    yield from self._run(images).unbind(0)
                if error is not None:
                    raise error

    def predict_to_dir(self, paths, output_path, verbose: bool = False):
        """Writes <stem>_<task>.png and <stem>_rgb.png for every path, as demo.py does; with `verbose` also its two lines per
        file, in input order.  An unreadable file raises what Image.open raises, after every earlier file has been written."""
        paths = [os.fspath(p) for p in paths]
        os.makedirs(output_path, exist_ok=True)
        writes = deque()   # (future, path, save_path) in input order

        def save(img, pixels, stem):
            pp.rgb_preview(img).save(os.path.join(output_path, f"{stem}_rgb.png"))
            Image.fromarray(pixels).save(os.path.join(output_path, f"{stem}_{self.task}.png"))

        def flush(everything):
            while writes and (everything or writes[0][0].done()):
                f, path, save_path = writes.popleft()
                f.result()
                if verbose:
                    print(f"Reading input {path} ...")
                    print(f"Writing output {save_path} ...")

        with ThreadPoolExecutor(self.workers) as pool:
            for first, images, error in self._batches(paths, pool):
                if images:
                    out = self._run(images)
                    host = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
                    host.copy_(out, non_blocking=True)
                    torch.cuda.current_stream(self.device).synchronize()
                    arr = host.numpy()
                    for j, img in enumerate(images):
                        path = paths[first + j]
                        stem = os.path.splitext(os.path.basename(path))[0]
                        save_path = os.path.join(output_path, f"{stem}_{self.task}.png")
                        writes.append((pool.submit(save, img, arr[j], stem), path, save_path))
                flush(error is not None)
                if error is not None:
                    if verbose:
                        print(f"Reading input {paths[first + len(images)]} ...")
                    raise error
            flush(True)
