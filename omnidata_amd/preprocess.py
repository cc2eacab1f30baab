"""Pre/post-processing of demo.py restated without torchvision (absent in this image).

Follows omnidata_tools/torch/demo.py:74-76,92-95 (Resize(384,BILINEAR) on the shorter side ->
CenterCrop(384) -> ToTensor [-> Normalize(0.5,0.5) for depth]), :101-102 (512 RGB preview),
:137-150 (grey -> 3 channels, clamp, ToPILImage / bicubic + 1-x + viridis).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image


def resize_shorter(img: Image.Image, size: int, resample=Image.BILINEAR) -> Image.Image:
    """torchvision Resize(size, resample) of a PIL image: the shorter side becomes `size`."""
    w, h = img.size
    if (w <= h and w == size) or (h <= w and h == size):
        return img
    if w < h:
        ow, oh = size, int(size * h / w)
    else:
        oh, ow = size, int(size * w / h)
    return img.resize((ow, oh), resample)


def center_crop(img: Image.Image, size: int) -> Image.Image:
    w, h = img.size
    if w < size or h < size:  # torchvision pads with 0 first
        pl, pt = max((size - w) // 2, 0), max((size - h) // 2, 0)
        canvas = Image.new(img.mode, (max(w, size), max(h, size)))
        canvas.paste(img, (pl, pt))
        img = canvas
        w, h = img.size
    top, left = int(round((h - size) / 2.0)), int(round((w - size) / 2.0))
    return img.crop((left, top, left + size, top + size))


def to_tensor(img: Image.Image) -> torch.Tensor:
    a = np.array(img)  # writable copy
    if a.ndim == 2:
        a = a[:, :, None]
    t = torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1)
    if t.dtype == torch.uint8:
        return t.float().div(255.0)
    return t.float()


def image_to_input(img: Image.Image, task: str, image_size: int = 384) -> torch.Tensor:
    """-> [1,3,384,384] fp32 in the model's input convention."""
    t = to_tensor(center_crop(resize_shorter(img, image_size), image_size))
    if task == "depth":
        t = (t - 0.5) / 0.5
    t = t[:3].unsqueeze(0)
    if t.shape[1] == 1:
        t = t.repeat_interleave(3, 1)
    return t


def rgb_preview(img: Image.Image) -> Image.Image:
    return center_crop(resize_shorter(img, 512), 512)


def normal_to_pil(output: torch.Tensor) -> Image.Image:
    """ToPILImage of a clamped [3,H,W] float tensor: mul(255).byte() (truncation)."""
    a = output.detach().cpu().clamp(0, 1).mul(255).byte().permute(1, 2, 0).numpy()
    return Image.fromarray(a)


def colorize_viridis(o: np.ndarray) -> np.ndarray:
    """plt.imsave(cmap='viridis') of a [H,W] array: normalise to the data range, apply the colormap, RGBA uint8."""
    from matplotlib import cm
    lo, hi = float(o.min()), float(o.max())
    n = (o - lo) / (hi - lo) if hi > lo else np.zeros_like(o)
    return (cm.get_cmap("viridis")(n) * 255).astype(np.uint8)


def depth_to_rgba(output: torch.Tensor) -> np.ndarray:
    """[1,H,W] or [H,W] clamped depth -> bicubic 512x512 -> clamp -> 1-x -> viridis RGBA uint8."""
    from matplotlib import cm
    o = output.detach().float().cpu().reshape(1, 1, *output.shape[-2:])
    o = F.interpolate(o, (512, 512), mode="bicubic").clamp(0, 1)
    o = (1 - o).squeeze().numpy()
    lo, hi = float(o.min()), float(o.max())  # plt.imsave normalises to [vmin, vmax] = data range
    n = (o - lo) / (hi - lo) if hi > lo else np.zeros_like(o)
    return (cm.get_cmap("viridis")(n) * 255).astype(np.uint8)


# ------------------------------------------------------------------ GPU path (libdptx.so prepost kernels)
def image_to_input_gpu(img, task: str, device="cuda:0") -> torch.Tensor:
    """Same result as image_to_input() (bit-identical), computed on the GPU from the raw uint8 pixels: only the
    undecoded image crosses PCIe.  RGB / greyscale uint8 images; other modes (RGBA is premultiplied by Pillow's
    resize) take the PIL path."""
    from ._native import call
    if isinstance(img, Image.Image):
        if img.mode not in ("RGB", "L"):
            return image_to_input(img, task).to(device)
        a = torch.from_numpy(np.array(img))
    else:
        a = img
    if a.dim() == 2:
        a = a[:, :, None]
    assert a.dtype == torch.uint8 and a.shape[2] in (1, 3)
    a = a.to(device).contiguous()
    H, W, C = a.shape
    x = torch.empty(1, 3, 384, 384, dtype=torch.float32, device=device)
    call("dptx_preprocess_u8", a.data_ptr(), H, W, C, W * C, int(task == "depth"), x.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return x


def normal_to_u8_gpu(output: torch.Tensor) -> torch.Tensor:
    """[3,384,384] float (cuda) -> [384,384,3] uint8 (cuda): clamp(0,1)*255 truncated, as ToPILImage does."""
    from ._native import call
    y = output.detach().float().contiguous()
    out = torch.empty(384, 384, 3, dtype=torch.uint8, device=y.device)
    call("dptx_postprocess_normal_u8", y.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out


def depth_to_512_gpu(output: torch.Tensor) -> torch.Tensor:
    """[384,384] float (cuda) -> [512,512] float (cuda): bicubic, clamp(0,1), 1-x (demo.py:143-145)."""
    from ._native import call
    y = output.detach().float().reshape(384, 384).contiguous()
    out = torch.empty(512, 512, dtype=torch.float32, device=y.device)
    call("dptx_postprocess_depth", y.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out


# ------------------------------------------------------------------ batches of images of different sizes (prepost_batch.hip)
import ctypes as _C

MAX_SCALE = 32       # include/dptx.h dptx_preprocess_u8_batch: shorter side <= 32 * S
MAX_SIDE = 16384


class ImageDesc(_C.Structure):
    """include/dptx.h dptx_image_desc."""
    _fields_ = [("offset", _C.c_int64), ("H", _C.c_int32), ("W", _C.c_int32), ("C", _C.c_int32), ("row_stride_bytes", _C.c_int32)]


def _as_hwc_u8(img) -> np.ndarray:
    a = np.asarray(img)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (1, 3):
        raise ValueError("pack_images takes uint8 HW, HW1 or HW3 pixel arrays (PIL images of mode L or RGB)")
    return np.ascontiguousarray(a)


def _supported(img, limit) -> bool:
    """Whether the batched resize kernels take this image: a PIL image of mode RGB / L or a uint8 HW / HW1 / HW3 array whose sides
    limit(h, w) accepts."""
    if isinstance(img, Image.Image):
        if img.mode not in ("RGB", "L"):
            return False
        w, h = img.size
    else:
        a = np.asarray(img) if not isinstance(img, torch.Tensor) else img
        if a.dtype not in (np.uint8, torch.uint8) or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)):
            return False
        h, w = a.shape[:2]
    return limit(h, w)


def batch_supported(img, image_size: int = 384) -> bool:
    """Whether dptx_preprocess_u8_batch takes this image (mode RGB / L inside the supported range); the others go through PIL."""
    return _supported(img, lambda h, w: 1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and min(h, w) <= MAX_SCALE * image_size)


def pack_images(images):
    """-> (buf, descs): one uint8 buffer (pinned when a GPU is present) that holds the pixel arrays of `images` (PIL RGB / L
    images or uint8 HW[C] arrays) back to back at 16-byte-aligned offsets, and the ctypes array of their dptx_image_desc."""
    arrays = [_as_hwc_u8(im) for im in images]
    descs = (ImageDesc * max(len(arrays), 1))()
    off = 0
    for i, a in enumerate(arrays):
        H, W, Cn = a.shape
        descs[i] = ImageDesc(off, H, W, Cn, W * Cn)
        off = (off + a.size + 15) // 16 * 16
    buf = torch.empty(max(off, 16), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    view = buf.numpy()
    for d, a in zip(descs, arrays):
        view[d.offset:d.offset + a.size] = a.reshape(-1)
    return buf, descs


def _as_pil(img) -> Image.Image:
    return img if isinstance(img, Image.Image) else Image.fromarray(np.asarray(img))


def _upload_and_resize(images, task: str, out_hw, device, supported, entry, unsupported: str, fallback, return_pixels: bool = False):
    """What images_to_input_gpu and images_to_input_rect_gpu share: the images `supported` accepts are packed, uploaded in one
    copy and resized by entry = (entry point, its workspace entry, the shape arguments both take after the count) -- straight
    into x when that is all of them, else scattered into their slots --; the others go through fallback(PIL image) -> [1,3,OH,OW].
    `unsupported` is the ValueError's text where the workspace entry rejects the shape.  return_pixels: see
    images_to_input_rect_gpu."""
    from ._native import MAX_DESCS, at, call, chunks, workspace
    images = list(images)
    B, (OH, OW) = len(images), out_hw
    device = torch.device(device)
    x = torch.empty(B, 3, OH, OW, dtype=torch.float32, device=device)
    if B == 0:
        return (x, torch.empty(16, dtype=torch.uint8, device=device), (ImageDesc * 1)()) if return_pixels else x
    fast = [i for i, im in enumerate(images) if supported(im)]
    slow = sorted(set(range(B)) - set(fast))
    dev = all_descs = None
    if return_pixels:   # one buffer with every image; the resize reads the descriptors of the images it takes
        buf, all_descs = pack_images([_as_pil(im).convert("RGB") if i in slow else im for i, im in enumerate(images)])
        descs = (ImageDesc * max(len(fast), 1))(*[all_descs[i] for i in fast])
        if not fast:
            with torch.cuda.device(device):
                dev = buf.to(device, non_blocking=True)
    elif fast:
        buf, descs = pack_images([images[i] for i in fast])
    if fast:
        name, ws_name, shape = entry
        ws = workspace(ws_name, device, (min(len(fast), MAX_DESCS), *shape), unsupported)
        with torch.cuda.device(device):
            dev = buf.to(device, non_blocking=True)
            stream = torch.cuda.current_stream().cuda_stream
            direct = len(fast) == B
            xf = x if direct else torch.empty(len(fast), 3, OH, OW, dtype=torch.float32, device=device)
            for b0, n in chunks(len(fast)):
                call(name, dev.data_ptr(), at(descs, b0), n, *shape, int(task == "depth"), xf[b0:].data_ptr(), ws.data_ptr(),
                     ws.numel(), stream)
            if not direct:
                x[torch.tensor(fast, device=device)] = xf
    for i in slow:
        x[i:i + 1] = fallback(_as_pil(images[i])).to(device)
    return (x, dev, all_descs) if return_pixels else x


def images_to_input_gpu(images, task: str, image_size: int = 384, device="cuda:0") -> torch.Tensor:
    """[B,3,S,S] fp32 on `device`: image_to_input() of every image (bit-identical), from ONE host->device copy of the raw
    pixels and one ragged-batch resize on the GPU.  Images the kernel does not take (other modes than RGB / L, sides outside
    its range) go through image_to_input() and are copied into their slot."""
    S = int(image_size)
    return _upload_and_resize(images, task, (S, S), device, lambda im: batch_supported(im, S),
                              ("dptx_preprocess_u8_batch", "dptx_preprocess_batch_workspace_bytes", (S,)),
                              f"image_size {S} is not a multiple of 32 in [32, 1024]", lambda im: image_to_input(im, task, S))


def normals_to_u8_gpu(output: torch.Tensor) -> torch.Tensor:
    """[B,3,S,S] float (cuda) -> [B,S,S,3] uint8 (cuda): clamp(0,1)*255 truncated, as ToPILImage does; one launch."""
    from ._native import call, check_cuda
    check_cuda("output", output)
    y = output.detach().float().contiguous()
    B, _, S, _ = y.shape
    out = torch.empty(B, S, S, 3, dtype=torch.uint8, device=y.device)
    with torch.cuda.device(y.device):
        call("dptx_postprocess_normal_u8_batch", y.data_ptr(), B, S, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out


def depths_to_512_gpu(output: torch.Tensor) -> torch.Tensor:
    """[B,S,S] (or [B,1,S,S]) float (cuda) -> [B,512,512] float (cuda): bicubic, clamp(0,1), 1-x per image; one launch."""
    from ._native import call, check_cuda
    check_cuda("output", output)
    S = output.shape[-1]
    y = output.detach().float().reshape(-1, S, S).contiguous()
    out = torch.empty(y.shape[0], 512, 512, dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        call("dptx_postprocess_depth_batch", y.data_ptr(), y.shape[0], S, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out


def viridis_lut() -> np.ndarray:
    """[256,4] uint8: the colormap entries plt.imsave looks up, scaled as colorize_viridis() scales them."""
    from matplotlib import cm
    return (cm.get_cmap("viridis")(np.arange(256)) * 255).astype(np.uint8)


def depths_to_rgba_gpu(maps: torch.Tensor) -> torch.Tensor:
    """[B,H,W] float (cuda) -> [B,H,W,4] uint8 (cuda): colorize_viridis() of every map (its own min / max), on the GPU."""
    from ._native import call, check_cuda, viridis_lut_on, workspace
    check_cuda("maps", maps)
    m = maps.detach().float().contiguous()
    B, N = m.shape[0], m[0].numel()
    lut = viridis_lut_on(m.device)
    ws = workspace("dptx_colorize_workspace_bytes", m.device, (B, N), f"colorize: unsupported shape {tuple(m.shape)}")
    out = torch.empty(*m.shape, 4, dtype=torch.uint8, device=m.device)
    with torch.cuda.device(m.device):
        call("dptx_colorize_u8_batch", m.data_ptr(), lut.data_ptr(), B, N, out.data_ptr(), ws.data_ptr(), ws.numel(),
             torch.cuda.current_stream().cuda_stream)
    return out


# ------------------------------------------------------------------ full-frame inference (fullframe.hip)
MAX_NET_SIDE = 1024          # include/dptx.h dptx_preprocess_u8_rect_batch: OH, OW <= 1024
MAX_NET_ELEMS = 2 ** 31      # the engine indexes one image's 256-channel maps with 32 bits: net_h * net_w * 256 < 2^31
RESIZE_MODES = {"normal_u8": 1, "normal_f32": 2, "depth_f32": 3, "depth_rgba": 4}   # include/dptx.h DPTX_RESIZE_*
RESIZE_RENORM = 16


def full_frame_size(w: int, h: int, size: int = 384, multiple: int = 32):
    """-> (net_w, net_h): the reference's Resize(size, size, keep_aspect_ratio=True, ensure_multiple_of=multiple,
    resize_method='lower_bound').get_size(w, h) (modules/midas/transforms.py:94-160): one scale, max(size / w, size / h), for
    both sides; each side rounded (half to even, as np.round) to a multiple, and up where that falls below `size`."""
    scale = max(size / w, size / h)

    def constrain(x):
        y = int(round(x / multiple) * multiple)
        if y < size:
            y = int(math.ceil(x / multiple) * multiple)
        return y
    return constrain(scale * w), constrain(scale * h)


def full_frame_net_size(w: int, h: int, size: int = 384, multiple: int = 32):
    """-> (net_w, net_h, capped): full_frame_size() with the long side cut back to what the kernels and the engine take
    (a side <= 1024, net_h * net_w * 256 < 2^31); `capped` says whether that changed anything."""
    nw, nh = full_frame_size(w, h, size, multiple)
    top = MAX_NET_SIDE // multiple * multiple
    cw, ch = min(nw, top), min(nh, top)
    while cw * ch * 256 >= MAX_NET_ELEMS:      # not reached with sides <= 1024; kept with the rule it states
        if cw >= ch:
            cw -= multiple
        else:
            ch -= multiple
    return cw, ch, (cw, ch) != (nw, nh)


def image_to_input_rect(img: Image.Image, task: str, net_hw) -> torch.Tensor:
    """-> [1,3,OH,OW] fp32: the whole image resized to the network's size (no crop), in the model's input convention."""
    OH, OW = net_hw
    t = to_tensor(img.resize((OW, OH), Image.BILINEAR))
    if task == "depth":
        t = (t - 0.5) / 0.5
    t = t[:3].unsqueeze(0)
    if t.shape[1] == 1:
        t = t.repeat_interleave(3, 1)
    return t


def rect_supported(img, net_hw) -> bool:
    """Whether dptx_preprocess_u8_rect_batch takes this image for the target (OH, OW); the others go through PIL."""
    OH, OW = net_hw
    return _supported(img, lambda h, w: 1 <= h <= min(MAX_SIDE, MAX_SCALE * OH) and 1 <= w <= min(MAX_SIDE, MAX_SCALE * OW))


def images_to_input_rect_gpu(images, task: str, net_hw, device="cuda:0", return_pixels: bool = False):
    """[B,3,OH,OW] fp32 on `device`: image_to_input_rect() of every image (bit-identical), from ONE host->device copy of the raw
    pixels and one ragged-batch resize on the GPU.  Images the kernel does not take go through PIL into their slot.
    return_pixels=True -> (x, pixels_dev, descs): also the uploaded uint8 pixel buffer and the ImageDesc array of ALL B images in
    input order, for guided_outputs_gpu; an image that takes the PIL path is packed as img.convert("RGB").  x is the same."""
    hw = (int(net_hw[0]), int(net_hw[1]))
    return _upload_and_resize(images, task, hw, device, lambda im: rect_supported(im, hw),
                              ("dptx_preprocess_u8_rect_batch", "dptx_preprocess_rect_batch_workspace_bytes", hw),
                              f"network size {hw}: both sides must be multiples of 32 in [64, 1024]",
                              lambda im: image_to_input_rect(im, task, hw), return_pixels)


def output_layout(sizes, mode: str):
    """-> (descs, total bytes): the packed output buffer dptx_postprocess_resize_batch fills for outputs of `sizes`
    [(H, W), ...]: tight rows, every output at a 16-byte-aligned offset."""
    bpp = 3 if mode == "normal_u8" else 4
    planes = 3 if mode == "normal_f32" else 1
    descs = (ImageDesc * max(len(sizes), 1))()
    off = 0
    for i, (H, W) in enumerate(sizes):
        descs[i] = ImageDesc(off, int(H), int(W), 3 if mode.startswith("normal") else 1, int(W) * bpp)
        off = (off + planes * int(H) * int(W) * bpp + 15) // 16 * 16
    return descs, off


def _one_of(name: str, value, allowed) -> None:
    """ValueError('<name> must be "a" or "b"') -- 'one of [...]' for more than two -- unless value is one of `allowed`."""
    if value not in allowed:
        names = [f'"{a}"' if isinstance(a, str) else str(a) for a in allowed]
        raise ValueError(f"{name} must be " + (" or ".join(names) if len(names) == 2 else f"one of {sorted(allowed)}"))


def _int_sizes(sizes):
    return [(int(H), int(W)) for H, W in sizes]


def _packed_outputs(sizes, mode: str, device):
    """-> (descs, out): output_layout() of `sizes` and the uint8 device buffer it describes; _output_views() slices it."""
    descs, total = output_layout(sizes, mode)
    return descs, torch.empty(max(total, 16), dtype=torch.uint8, device=device)


def _resize_code(mode: str, renormalize: bool) -> int:
    """The mode argument of the resize and guided entry points; ValueError for an unknown mode or renormalize on depth."""
    _one_of("mode", mode, RESIZE_MODES)
    if renormalize and not mode.startswith("normal"):
        raise ValueError("renormalize applies to surface normals only")
    return RESIZE_MODES[mode] | (RESIZE_RENORM if renormalize else 0)


def _resize_outputs(sizes, mode: str, code: int, device, ws_entry: str):
    """-> (descs, out, (lut pointer, workspace pointer, workspace bytes)): the packed outputs of `sizes`, whose sides are checked,
    and what depth_rgba needs besides, the colormap and the workspace of the range pass (zeros for the other modes)."""
    from ._native import MAX_DESCS, viridis_lut_on, workspace
    if any(not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE) for H, W in sizes):
        raise ValueError(f"output sides must be in [1, {MAX_SIDE}]")
    descs, out = _packed_outputs(sizes, mode, device)
    if mode != "depth_rgba":
        return descs, out, (0, 0, 0)
    ws = workspace(ws_entry, device, (min(len(sizes), MAX_DESCS), code), "unsupported mode")
    return descs, out, (viridis_lut_on(device).data_ptr(), ws.data_ptr(), ws.numel())


def resize_outputs_gpu(y: torch.Tensor, sizes, mode: str, renormalize: bool = False):
    """y [B,3,h,w] (normal_*) or [B,h,w] / [B,1,h,w] (depth_*) float (cuda), sizes [(H, W)] * B -> list of B device tensors
    (views of one packed buffer), output i at its own size: normal_u8 [H,W,3] uint8, normal_f32 [3,H,W] fp32, depth_f32 [H,W]
    fp32, depth_rgba [H,W,4] uint8 (viridis over the map's own range).  One entry-point call per 4096 outputs."""
    from ._native import at, call, check_cuda, chunks
    check_cuda("y", y)
    code = _resize_code(mode, renormalize)
    h, w = y.shape[-2:]
    y = y.detach().float().reshape(-1, 3 if mode.startswith("normal") else 1, h, w).contiguous()
    sizes = _int_sizes(sizes)
    B = y.shape[0]
    if len(sizes) != B:
        raise ValueError(f"{B} maps but {len(sizes)} sizes")
    if B == 0:
        return []
    descs, out, tail = _resize_outputs(sizes, mode, code, y.device, "dptx_postprocess_resize_workspace_bytes")
    with torch.cuda.device(y.device):
        stream = torch.cuda.current_stream().cuda_stream
        for b0, n in chunks(B):
            call("dptx_postprocess_resize_batch", y[b0:].data_ptr(), n, y.shape[1], h, w, at(descs, b0), code, out.data_ptr(), *tail,
                 stream)
    return _output_views(out, descs, sizes, mode)


def _output_views(out: torch.Tensor, descs, sizes, mode: str):
    """The outputs inside the packed buffer that output_layout() describes, as tensors."""
    res = []
    for d, (H, W) in zip(descs, sizes):
        if mode == "normal_u8":
            res.append(out[d.offset:d.offset + H * W * 3].view(H, W, 3))
        elif mode == "normal_f32":
            res.append(out[d.offset:d.offset + 12 * H * W].view(torch.float32).view(3, H, W))
        elif mode == "depth_f32":
            res.append(out[d.offset:d.offset + 4 * H * W].view(torch.float32).view(H, W))
        else:
            res.append(out[d.offset:d.offset + 4 * H * W].view(H, W, 4))
    return res


# ------------------------------------------------------------------ guided upsampling (guided.hip)
class GuidedParams(_C.Structure):
    """include/dptx.h dptx_guided_params."""
    _fields_ = [("radius", _C.c_int32), ("sigma_space", _C.c_float), ("sigma_range", _C.c_float)]


def guided_params(options=None) -> dict:
    """-> {radius, sigma_space, sigma_range} with the defaults (2, 1.0, 0.1) filled in; ValueError for an unknown name, a radius
    outside {1, 2, 3} or a sigma that is not a positive finite number."""
    p = dict(radius=2, sigma_space=1.0, sigma_range=0.1)
    if not isinstance(options or {}, dict) or set(options or {}) - set(p):
        raise ValueError("guided must be None, True or a dict of radius, sigma_space, sigma_range")
    p.update(options or {})
    if isinstance(p["radius"], bool) or p["radius"] not in (1, 2, 3):
        raise ValueError("guided: radius must be 1, 2 or 3")
    for name in ("sigma_space", "sigma_range"):
        v = p[name]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (0 < v < math.inf):
            raise ValueError(f"guided: {name} must be a positive number")
    return dict(radius=int(p["radius"]), sigma_space=float(p["sigma_space"]), sigma_range=float(p["sigma_range"]))


def guided_outputs_gpu(y: torch.Tensor, guide_lo: torch.Tensor, pixels_dev: torch.Tensor, descs, sizes, mode: str,
                       renormalize: bool = False, radius: int = 2, sigma_space: float = 1.0, sigma_range: float = 0.1):
    """resize_outputs_gpu with guided (joint bilateral, Kopf et al. 2007) upsampling instead of the plain interpolation: the same
    arguments y, sizes, mode, renormalize and the same list of views, output i at its own size H x W.

    y [B,3,h,w] (normal_*) or [B,h,w] / [B,1,h,w] (depth_*), already clamped to [0, 1]; guide_lo [B,3,h,w] in [0, 1]: the image as
    the network saw it (the network input x for normals, x * 0.5 + 0.5 for depth); pixels_dev / descs: the packed uint8 pixels on
    the device and their ImageDesc (pack_images; images_to_input_rect_gpu(..., return_pixels=True)), image i of size sizes[i], one
    or three channels (a grey image counts three times), g = u8 / 255.

    Output pixel (Y, X), all in fp32, every operation rounded on its own:
      sy = (h / H) * (Y + 0.5) - 0.5, sx likewise (ATen's align_corners=False coordinate, not clamped); by, bx = their floors;
      taps qy in by - R + 1 .. by + R, qx in bx - R + 1 .. bx + R, those outside the map skipped (at least one is inside);
      e_q = ks * ((qy - sy)^2 + (qx - sx)^2) + kr * sum_c (G_hi[c](Y, X) - G_lo[c](qy, qx))^2 with ks = 1 / (2 sigma_space^2),
      kr = 1 / (2 sigma_range^2); w_q = exp(-(e_q - min e)), so the largest weight is 1;
      v_c = sum_q w_q * S_c(q) / sum_q w_q in (qy, qx) order; then the mode's steps of resize_outputs_gpu (renormalize, clamp and
      quantisation; depth: clamp, 1 - x; depth_rgba: viridis over the map's own range).
    radius R in {1, 2, 3}, sigma_space in low-resolution pixels, sigma_range in [0, 1] colour units.  include/dptx.h ("Guided
    upsampling") is the full statement.  One entry-point call per 4096 outputs; bitwise reproducible, independent of the batch."""
    from ._native import at, call, check_cuda, chunks
    check_cuda("y", y)
    check_cuda("guide_lo", guide_lo)
    check_cuda("pixels_dev", pixels_dev)
    code = _resize_code(mode, renormalize)
    params = GuidedParams(**guided_params(dict(radius=radius, sigma_space=sigma_space, sigma_range=sigma_range)))
    h, w = y.shape[-2:]
    y = y.detach().float().reshape(-1, 3 if mode.startswith("normal") else 1, h, w).contiguous()
    B = y.shape[0]
    if tuple(guide_lo.shape) != (B, 3, h, w):
        raise ValueError(f"guide_lo must be [{B}, 3, {h}, {w}], the maps' resolution; got {tuple(guide_lo.shape)}")
    guide_lo = guide_lo.detach().float().contiguous()
    if pixels_dev.dtype != torch.uint8 or not pixels_dev.is_contiguous() or guide_lo.device != y.device or pixels_dev.device != y.device:
        raise ValueError("pixels_dev must be a contiguous uint8 tensor, and the guides must be on the maps' device")
    sizes = _int_sizes(sizes)
    if len(sizes) != B or len(descs) < B:
        raise ValueError(f"{B} maps but {len(sizes)} sizes and {len(descs)} guide descriptors")
    if B == 0:
        return []
    outs, out, tail = _resize_outputs(sizes, mode, code, y.device, "dptx_postprocess_guided_workspace_bytes")
    for i, (H, W) in enumerate(sizes):
        d = descs[i]
        if (d.H, d.W) != (H, W) or d.C not in (1, 3) or d.row_stride_bytes < d.W * d.C or d.offset < 0 or \
                d.offset + (d.H - 1) * d.row_stride_bytes + d.W * d.C > pixels_dev.numel():
            raise ValueError(f"guide {i}: a {d.H}x{d.W}x{d.C} image at offset {d.offset} does not describe {H}x{W} pixels inside pixels_dev")
    with torch.cuda.device(y.device):
        stream = torch.cuda.current_stream().cuda_stream
        for b0, n in chunks(B):
            call("dptx_postprocess_guided_batch", y[b0:].data_ptr(), guide_lo[b0:].data_ptr(), n, y.shape[1], h, w,
                 pixels_dev.data_ptr(), at(descs, b0), at(outs, b0), _C.addressof(params), code, out.data_ptr(), *tail, stream)
    return _output_views(out, outs, sizes, mode)


# ------------------------------------------------------------------ test-time augmentation (fullframe.hip views entry, tta.hip, tta_depth.hip)
TTA_MEAN = 32                # include/dptx.h DPTX_TTA_MEAN
TTA_RAW_VIEWS = 64           # include/dptx.h DPTX_TTA_RAW_VIEWS
TTA_MAX_VIEWS = 64           # include/dptx.h DPTX_TTA_MAX_VIEWS: views per image


class TtaView(_C.Structure):
    """include/dptx.h dptx_tta_view."""
    _fields_ = [("offset", _C.c_int64), ("h", _C.c_int32), ("w", _C.c_int32), ("image", _C.c_int32), ("y0", _C.c_int32),
                ("x0", _C.c_int32), ("ch", _C.c_int32), ("cw", _C.c_int32), ("flip", _C.c_int32)]


def window_desc(d: ImageDesc, box) -> ImageDesc:
    """The descriptor of the window box = (left, top, right, bottom) of the image d describes, as PIL's img.crop(box) cuts it:
    the parent's row stride, the offset of the window's first pixel.  The pixels are not copied."""
    left, top, right, bottom = (int(v) for v in box)
    if not (0 <= left < right <= d.W and 0 <= top < bottom <= d.H):
        raise ValueError(f"window {box} is not inside the {d.W}x{d.H} image")
    return ImageDesc(d.offset + top * d.row_stride_bytes + left * d.C, bottom - top, right - left, d.C, d.row_stride_bytes)


def views_to_input_gpu(pixels_dev: torch.Tensor, descs, flips, net_hw, task: str = "normal") -> torch.Tensor:
    """[B,3,OH,OW] fp32: per descriptor ToTensor(ImageOps.mirror(window.resize((OW, OH), BILINEAR))) -- mirrored where flips[i]
    -- bit-identical to Pillow.  pixels_dev: the packed uint8 pixels on the device (pack_images, uploaded once); descs: ImageDesc
    of whole images or of windows of them (window_desc); flips: one truth value per descriptor, or None.  One entry-point call
    per 4096 views (dptx_preprocess_u8_views_batch)."""
    from ._native import MAX_DESCS, at, call, check_cuda, chunks, workspace
    check_cuda("pixels_dev", pixels_dev)
    descs = list(descs)
    B, (OH, OW) = len(descs), (int(net_hw[0]), int(net_hw[1]))
    x = torch.empty(B, 3, OH, OW, dtype=torch.float32, device=pixels_dev.device)
    if B == 0:
        return x
    if flips is not None and len(flips) != B:
        raise ValueError(f"{B} views but {len(flips)} flips")
    arr = (ImageDesc * B)(*descs)
    fl = (_C.c_uint8 * B)(*[1 if f else 0 for f in flips]) if flips is not None else None
    ws = workspace("dptx_preprocess_rect_batch_workspace_bytes", pixels_dev.device, (min(B, MAX_DESCS), OH, OW),
                   f"network size {(OH, OW)}: both sides must be multiples of 32 in [64, 1024]")
    with torch.cuda.device(pixels_dev.device):
        stream = torch.cuda.current_stream().cuda_stream
        for b0, n in chunks(B):
            call("dptx_preprocess_u8_views_batch", pixels_dev.data_ptr(), at(arr, b0), at(fl, b0) if fl is not None else None, n, OH, OW,
                 int(task == "depth"), x[b0:].data_ptr(), ws.data_ptr(), ws.numel(), stream)
    return x


def merge_normal_views_gpu(maps: torch.Tensor, views, sizes, merger: str = "median", normalize_views: bool = True,
                           output: str = "u8"):
    """The merge of test-time augmentation (dptx_tta_merge_normals), one call: maps is ONE fp32 cuda tensor that holds every
    view's [3,h,w] map (values as the network returns them, in [0, 1]); views is a sequence of TtaView -- offset in BYTES into
    maps, the views of an image consecutive, images ascending --; sizes [(H, W)] per output image.  Per pixel the views that
    cover it are decoded (2m - 1), normalised at their own resolution (normalize_views), resized into their windows
    (F.interpolate bilinear; a flipped view un-mirrored with x negated), merged per channel by np.median ("median") or the mean
    in view order ("mean"), normalised again and encoded.  -> list of device tensors (views of one packed buffer): [H,W,3] uint8
    (output "u8") or [3,H,W] fp32 ("f32"); a pixel no view covers is the zero vector (0.5 / 127)."""
    from ._native import call
    _check_maps(maps)
    _one_of("merger", merger, ("median", "mean"))
    _one_of("output", output, ("u8", "f32"))
    views = list(views)
    sizes = _int_sizes(sizes)
    if not sizes:
        return []
    mode = "normal_u8" if output == "u8" else "normal_f32"
    _check_maps(maps, views, lambda v: [(v.offset, 12 * v.h * v.w, "a view lies outside maps")])
    descs, out = _packed_outputs(sizes, mode, maps.device)
    code = RESIZE_MODES[mode] | (TTA_MEAN if merger == "mean" else 0) | (0 if normalize_views else TTA_RAW_VIEWS)
    arr = (TtaView * max(len(views), 1))(*views)
    with torch.cuda.device(maps.device):
        call("dptx_tta_merge_normals", maps.data_ptr(), _C.addressof(arr), len(views), _C.addressof(descs), len(sizes), code,
             out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return _output_views(out, descs, sizes, mode)


def _check_maps(maps, items=(), spans=None):
    """maps must be a contiguous fp32 CUDA tensor, and every (offset, bytes, message) that spans(item) lists must lie inside it:
    ValueError(message) otherwise.  -> the items as a list."""
    from ._native import check_cuda
    check_cuda("maps", maps)
    if maps.dtype != torch.float32 or not maps.is_contiguous():
        raise ValueError("maps must be a contiguous fp32 tensor")
    items = list(items)
    for item in items:
        for offset, nbytes, message in spans(item):
            if offset < 0 or offset + nbytes > maps.numel() * 4:
                raise ValueError(message)
    return items


def _check_depth_views(maps, views, sizes):
    return _check_maps(maps, views, lambda v: [(v.offset, 4 * v.h * v.w, "a view lies outside maps")]), _int_sizes(sizes)


def _check_coeffs(coeffs, rows: int, message: str) -> None:
    from ._native import check_cuda
    if coeffs is not None:
        check_cuda("coeffs", coeffs)
        if coeffs.dtype != torch.float32 or not coeffs.is_contiguous() or tuple(coeffs.shape) != (rows, 2):
            raise ValueError(message)


def _depth_views(out: torch.Tensor, descs, sizes, output: str):
    """The depth writers' outputs: the fp32 maps inside the packed buffer, or with output "rgba" depths_to_rgba_gpu of each."""
    res = _output_views(out, descs, sizes, "depth_f32")
    return [depths_to_rgba_gpu(m[None])[0] for m in res] if output == "rgba" else res


def align_depth_views_gpu(maps: torch.Tensor, views, anchors, sizes):
    """The alignment step of test-time augmentation for depth (dptx_tta_align_depth), one call: maps is ONE fp32 cuda tensor
    that holds every view's [1,h,w] map as the network returns it; views is a sequence of TtaView as merge_normal_views_gpu
    takes it; anchors[i] is the index (into views) of the view of image i that covers the whole image; sizes [(H, W)] per
    image.  Every view is fitted to its image's anchor by least squares over its window (include/dptx.h: fp64 sums, solved in
    fp64); the anchor's coefficients are exactly (1, 0).  -> (coeffs [n_views, 2] cuda fp32: scale, shift; the workspace the
    call wrote, for merge_depth_views_gpu)."""
    from ._native import call
    views, sizes = _check_depth_views(maps, views, sizes)
    anchors = [int(a) for a in anchors]
    if len(anchors) != len(sizes):
        raise ValueError(f"{len(sizes)} images but {len(anchors)} anchors")
    if not sizes:
        raise ValueError("no image")
    descs, _ = output_layout(sizes, "depth_f32")
    arr = (TtaView * max(len(views), 1))(*views)
    anc = (_C.c_int32 * len(anchors))(*anchors)
    nbytes = _C.c_int64()
    call("dptx_tta_depth_workspace_bytes", _C.addressof(arr), len(views), _C.addressof(descs), len(sizes), _C.byref(nbytes))
    ws = torch.empty(max(nbytes.value, 256), dtype=torch.uint8, device=maps.device)
    coeffs = torch.empty(len(views), 2, dtype=torch.float32, device=maps.device)
    with torch.cuda.device(maps.device):
        call("dptx_tta_align_depth", maps.data_ptr(), _C.addressof(arr), len(views), _C.addressof(anc), _C.addressof(descs),
             len(sizes), coeffs.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    return coeffs, ws


def merge_depth_views_gpu(maps: torch.Tensor, views, sizes, coeffs=None, ws=None, merger: str = "median", output: str = "f32"):
    """The merge of test-time augmentation for depth (dptx_tta_merge_depth), one call: per pixel the views that cover it are
    clamped to [0, 1] at their own resolution, resized into their windows (F.interpolate bilinear; a flipped view un-mirrored),
    mapped by their coefficients (scale * r + shift; coeffs / ws as align_depth_views_gpu returned them, None = unaligned) and
    merged by np.median ("median") or the mean in view order ("mean"); then clamp(0, 1) and 1 - x.  -> list of device tensors:
    [H,W] fp32 (output "f32", views of one packed buffer) or [H,W,4] uint8 ("rgba": depths_to_rgba_gpu of each map, viridis over
    its own range, as the full-frame depth path writes)."""
    from ._native import call
    views, sizes = _check_depth_views(maps, views, sizes)
    _one_of("merger", merger, ("median", "mean"))
    _one_of("output", output, ("f32", "rgba"))
    if not sizes:
        return []
    _check_coeffs(coeffs, len(views), "coeffs must be a contiguous fp32 tensor [n_views, 2]")
    descs, out = _packed_outputs(sizes, "depth_f32", maps.device)
    code = RESIZE_MODES["depth_f32"] | (TTA_MEAN if merger == "mean" else 0)
    arr = (TtaView * max(len(views), 1))(*views)
    with torch.cuda.device(maps.device):
        call("dptx_tta_merge_depth", maps.data_ptr(), _C.addressof(arr), len(views), coeffs.data_ptr() if coeffs is not None else None,
             _C.addressof(descs), len(sizes), code, out.data_ptr(), ws.data_ptr() if ws is not None else None,
             torch.cuda.current_stream().cuda_stream)
    return _depth_views(out, descs, sizes, output)


# ------------------------------------------------------------------ tiled inference (tiles.hip; omnidata_amd/tiled.py states the protocol)
TILE_MAX_AXIS = 64           # include/dptx.h DPTX_TILE_MAX_AXIS: tiles per axis


class TileGrid(_C.Structure):
    """include/dptx.h dptx_tile_grid: one per image.  make() fills it from Python lists."""
    _fields_ = [("offset", _C.c_int64), ("anchor_offset", _C.c_int64), ("h", _C.c_int32), ("w", _C.c_int32), ("ch", _C.c_int32),
                ("cw", _C.c_int32), ("ny", _C.c_int32), ("nx", _C.c_int32), ("ramp_y", _C.c_int32), ("ramp_x", _C.c_int32),
                ("ah", _C.c_int32), ("aw", _C.c_int32), ("y0", _C.c_int32 * 64), ("x0", _C.c_int32 * 64)]

    @classmethod
    def make(cls, offset, net_hw, window_hw, ys, xs, ramps=(0, 0), anchor_offset=-1, anchor_hw=(0, 0)):
        """offset / anchor_offset: bytes into maps; net_hw (h, w); window_hw (ch, cw); ys / xs: the starts; ramps (ramp_y, ramp_x)."""
        ys, xs = [int(v) for v in ys], [int(v) for v in xs]
        if not (1 <= len(ys) <= TILE_MAX_AXIS and 1 <= len(xs) <= TILE_MAX_AXIS):
            raise ValueError(f"a grid has 1..{TILE_MAX_AXIS} tiles per axis, not {len(ys)} x {len(xs)}")
        g = cls(int(offset), int(anchor_offset), int(net_hw[0]), int(net_hw[1]), int(window_hw[0]), int(window_hw[1]), len(ys), len(xs),
                int(ramps[0]), int(ramps[1]), int(anchor_hw[0]), int(anchor_hw[1]))
        g.y0[:len(ys)] = ys
        g.x0[:len(xs)] = xs
        return g

    @property
    def tiles(self) -> int:
        return self.ny * self.nx


def _check_tile_maps(maps, grids, sizes, channels, anchors=False):
    def spans(g):
        return [(g.offset, 4 * channels * g.h * g.w * g.tiles, "a grid's tiles lie outside maps")] + \
            ([(g.anchor_offset, 4 * g.ah * g.aw, "a grid's anchor lies outside maps")] if anchors else [])

    _check_maps(maps)
    grids, sizes = list(grids), _int_sizes(sizes)
    if len(grids) != len(sizes):
        raise ValueError(f"{len(sizes)} images but {len(grids)} grids")
    return _check_maps(maps, grids, spans), sizes


def blend_normal_tiles_gpu(maps: torch.Tensor, grids, sizes, normalize_views: bool = True, output: str = "u8"):
    """The blend of tiled inference for surface normals (dptx_tile_blend_normals), one call: maps is ONE fp32 cuda tensor that holds
    every tile's [3,h,w] map, an image's tiles contiguous in grid order from grids[i].offset (bytes); grids: one TileGrid per
    image; sizes [(H, W)] per image.  Every tile is decoded (2m - 1), normalised at its own resolution (normalize_views), resized
    into its window and weighted with the feathered ramp of include/dptx.h; the weighted sum is normalised again and encoded.
    -> list of device tensors (views of one packed buffer): [H,W,3] uint8 (output "u8") or [3,H,W] fp32 ("f32")."""
    from ._native import call
    grids, sizes = _check_tile_maps(maps, grids, sizes, 3)
    _one_of("output", output, ("u8", "f32"))
    if not sizes:
        return []
    mode = "normal_u8" if output == "u8" else "normal_f32"
    descs, out = _packed_outputs(sizes, mode, maps.device)
    code = RESIZE_MODES[mode] | (0 if normalize_views else TTA_RAW_VIEWS)
    arr = (TileGrid * len(grids))(*grids)
    with torch.cuda.device(maps.device):
        call("dptx_tile_blend_normals", maps.data_ptr(), _C.addressof(arr), _C.addressof(descs), len(sizes), code, out.data_ptr(),
             torch.cuda.current_stream().cuda_stream)
    return _output_views(out, descs, sizes, mode)


def align_depth_tiles_gpu(maps: torch.Tensor, grids, sizes):
    """The alignment step of tiled depth inference (dptx_tile_align_depth), one call: every tile of every grid is fitted to its
    image's anchor -- the whole image's [1,ah,aw] map at grids[i].anchor_offset -- by the least squares of align_depth_views_gpu
    (the same device code, the same bits).  -> coeffs [tiles of all images, 2] cuda fp32 (scale, shift), image-major, an image's
    tiles in grid order."""
    from ._native import call
    grids, sizes = _check_tile_maps(maps, grids, sizes, 1, anchors=True)
    if not sizes:
        raise ValueError("no image")
    descs, _ = output_layout(sizes, "depth_f32")
    arr = (TileGrid * len(grids))(*grids)
    nbytes = _C.c_int64()
    call("dptx_tile_depth_workspace_bytes", _C.addressof(arr), _C.addressof(descs), len(sizes), _C.byref(nbytes))
    ws = torch.empty(max(nbytes.value, 256), dtype=torch.uint8, device=maps.device)
    coeffs = torch.empty(sum(g.tiles for g in grids), 2, dtype=torch.float32, device=maps.device)
    with torch.cuda.device(maps.device):
        call("dptx_tile_align_depth", maps.data_ptr(), _C.addressof(arr), _C.addressof(descs), len(sizes), coeffs.data_ptr(),
             ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    return coeffs


def blend_depth_tiles_gpu(maps: torch.Tensor, grids, sizes, coeffs=None, output: str = "f32"):
    """The blend of tiled depth inference (dptx_tile_blend_depth), one call: every tile is clamped to [0, 1] at its own resolution,
    resized into its window, mapped by its coefficients (scale * r + shift; coeffs as align_depth_tiles_gpu returned them, None =
    unaligned, for comparison) and weighted with the feathered ramp; sum / weight sum, clamp(0, 1), 1 - x.  The anchors are not
    blended.  -> list of device tensors: [H,W] fp32 (output "f32", views of one packed buffer) or [H,W,4] uint8 ("rgba": viridis
    over the map's own range, as the full-frame depth path writes)."""
    from ._native import call
    grids, sizes = _check_tile_maps(maps, grids, sizes, 1)
    _one_of("output", output, ("f32", "rgba"))
    if not sizes:
        return []
    _check_coeffs(coeffs, sum(g.tiles for g in grids), "coeffs must be a contiguous fp32 tensor [tiles, 2]")
    descs, out = _packed_outputs(sizes, "depth_f32", maps.device)
    arr = (TileGrid * len(grids))(*grids)
    with torch.cuda.device(maps.device):
        call("dptx_tile_blend_depth", maps.data_ptr(), _C.addressof(arr), coeffs.data_ptr() if coeffs is not None else None,
             _C.addressof(descs), len(sizes), RESIZE_MODES["depth_f32"], out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return _depth_views(out, descs, sizes, output)
