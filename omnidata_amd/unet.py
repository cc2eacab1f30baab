"""The reference's version-1 UNet (omnidata_tools/torch/modules/unet.py:57-105; checkpoint omnidata_unet_normal_v1.pth)
behind libdptx.so: ``UNet`` keeps the constructor, the state-dict key names and shapes and the forward contract of the
reference's module, but the forward runs in hand-written gfx950 kernels (csrc/unet.hip, csrc/unet_engine.hip).

No CPU / eager fallback: CPU tensors, a missing GPU or a missing library raise.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from .engine import DTYPES, ERRORS, IO_DTYPES, _stream, load_library

DOWNSAMPLE = 6


class DptxUnetConfig(C.Structure):
    _fields_ = [("out_channels", C.c_int32), ("max_batch", C.c_int32), ("dtype", C.c_int32), ("device_id", C.c_int32),
                ("max_height", C.c_int32), ("max_width", C.c_int32), ("reserved", C.c_int32 * 2)]


def unet_state_dict_spec(out_channels: int = 3) -> "OrderedDict[str, tuple]":
    """{key: shape} of the reference's UNet(downsample=6, in_channels=3, out_channels) in state-dict order (174 keys)."""
    spec: "OrderedDict[str, tuple]" = OrderedDict()

    def conv(name, cin, cout, k=3):
        spec[name + ".weight"] = (cout, cin, k, k)
        spec[name + ".bias"] = (cout,)

    def norm(name, c):
        spec[name + ".weight"] = (c,)
        spec[name + ".bias"] = (c,)

    def block(pre, cin, cout):
        for j in (1, 2, 3):
            conv(f"{pre}.conv{j}", cin if j == 1 else cout, cout)
            norm(f"{pre}.bn{j}", cout)

    block("down1", 3, 16)
    for i in range(DOWNSAMPLE):
        block(f"down_blocks.{i}", 16 << i, 32 << i)
    for j in (1, 2, 3):
        conv(f"mid_conv{j}", 1024, 1024)
        norm(f"bn{j}", 1024)
    for i in range(DOWNSAMPLE):
        block(f"up_blocks.{i}", 48 << i, 16 << i)
    conv("last_conv1", 16, 16)
    norm("last_bn", 16)
    conv("last_conv2", 16, out_channels, 1)
    return spec


def unet_init_state_dict(seed: int, out_channels: int = 3) -> Dict[str, torch.Tensor]:
    """Seeded initial weights (He-scaled convolutions, norm weights 1, norm biases 0): activations stay O(1)."""
    g = torch.Generator().manual_seed(4000 + int(seed))
    sd = OrderedDict()
    for k, shape in unet_state_dict_spec(out_channels).items():
        if len(shape) == 4:
            sd[k] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        elif k.endswith(".weight"):
            sd[k] = torch.ones(shape)
        else:
            sd[k] = torch.zeros(shape)
    return sd


def strip_checkpoint(obj) -> Dict[str, torch.Tensor]:
    """The loading branch of the reference's demo.py:54-59: a ``{'state_dict': {'model.<key>': tensor}}`` checkpoint or a
    plain state dict -> plain state dict."""
    if isinstance(obj, dict) and "state_dict" in obj and isinstance(obj["state_dict"], dict):
        return OrderedDict((k.replace("model.", ""), v) for k, v in obj["state_dict"].items())
    return obj


class UNetEngine:
    """One dptx_unet handle: packed weights + activation arena on one GPU (device_id None: host-only packing)."""

    def __init__(self, out_channels: int = 3, max_batch: int = 32, dtype: str = "fp16", device_id: Optional[int] = 0,
                 max_hw=(384, 384)):
        self.lib = load_library()
        cfg = DptxUnetConfig()
        self.lib.dptx_unet_default_config(C.byref(cfg))
        if dtype not in DTYPES:
            raise ValueError(f"unknown dtype {dtype!r}")
        cfg.out_channels, cfg.max_batch, cfg.dtype = int(out_channels), int(max_batch), DTYPES[dtype]
        cfg.device_id = -1 if device_id is None else int(device_id)
        cfg.max_height, cfg.max_width = int(max_hw[0]), int(max_hw[1])
        self.cfg, self.dtype = cfg, dtype
        self.h = C.c_void_p()
        rc = self.lib.dptx_unet_create(C.byref(self.h), C.byref(cfg))
        if rc != 0:
            self.h = None
            raise RuntimeError(f"dptx_unet_create failed: {ERRORS.get(rc, rc)}"
                               + (" (no HIP device visible; the HIP path has no CPU fallback)" if rc == -4 else ""))

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({ERRORS.get(rc, rc)}): {self.lib.dptx_unet_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.dptx_unet_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_tensor(self, key: str, value: torch.Tensor) -> int:
        a = value.detach().to("cpu", torch.float32).contiguous().numpy()
        shape = (C.c_int64 * a.ndim)(*a.shape)
        return self.lib.dptx_unet_load_tensor(self.h, key.encode(), a.ctypes.data, shape, a.ndim)

    def load_state_dict(self, sd):
        for k, v in strip_checkpoint(sd).items():
            self._check(self.load_tensor(k, v), f"load_tensor({k})")
        self._check(self.lib.dptx_unet_finalize_weights(self.h), "finalize_weights")

    @property
    def packed_bytes(self) -> int:
        return self.lib.dptx_unet_packed_bytes(self.h)

    @property
    def device_bytes(self) -> int:
        return self.lib.dptx_unet_device_bytes(self.h)

    def packed_entry(self, key: str):
        off, n = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.dptx_unet_packed_entry(self.h, key.encode(), C.byref(off), C.byref(n)), f"packed_entry({key})")
        return off.value, n.value

    def export_packed_host(self) -> np.ndarray:
        buf = np.empty(self.packed_bytes, dtype=np.uint8)
        self._check(self.lib.dptx_unet_export_packed_host(self.h, buf.ctypes.data, buf.size), "export_packed_host")
        return buf

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, classes: int = 7) -> torch.Tensor:
        """x [B,3,H,W] CUDA fp32 / bf16 / fp16 -> [B,out,H,W] fp32, enqueued on the current stream."""
        if not x.is_cuda:
            raise RuntimeError("the UNet forward needs a CUDA(HIP) tensor; there is no CPU fallback")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected [B,3,H,W], got {tuple(x.shape)}")
        if x.dtype not in IO_DTYPES:
            x = x.float()
        x = x.contiguous()
        B, _, H, W = x.shape
        if out is None:
            out = torch.empty(B, self.cfg.out_channels, H, W, dtype=torch.float32, device=x.device)
        elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (B, self.cfg.out_channels, H, W):
            raise ValueError("out must be a contiguous fp32 tensor of the result's shape")
        st = _stream(x.device)
        if classes == 7:
            rc = self.lib.dptx_unet_forward(self.h, x.data_ptr(), out.data_ptr(), B, H, W, IO_DTYPES[x.dtype], st)
        else:
            rc = self.lib.dptx_unet_debug_forward_classes(self.h, x.data_ptr(), out.data_ptr(), B, H, W, IO_DTYPES[x.dtype], int(classes), st)
        self._check(rc, "forward")
        return out

    def range_overflowed(self, reset: bool = True) -> bool:
        v = C.c_int32(0)
        self._check(self.lib.dptx_unet_range_status(self.h, C.byref(v), int(reset), _stream(torch.device("cuda", self.cfg.device_id))),
                    "range_status")
        return bool(v.value)

    def arena_fill(self, byte_value: int):
        self._check(self.lib.dptx_unet_debug_arena_fill(self.h, int(byte_value)), "debug_arena_fill")


class _Node(nn.Module):
    """Anonymous container so that nested parameter names equal the reference's keys."""


class UNet(nn.Module):
    """Drop-in for the reference's ``UNet(downsample=6, in_channels=3, out_channels=3, patch_size=1)``, inference only.

    Parameters carry the reference's names and shapes, so ``load_state_dict`` of its checkpoint works -- also in the
    ``{'state_dict': {'model.<key>': ...}}`` form of the reference's demo.py.  The forward is engine-backed: the weights are
    pushed to the engine at the first forward and after every ``load_state_dict`` / ``.to()``.

    ``forward(x)``: [B,3,H,W] CUDA fp32 (or fp16 / bf16) in [0, 1] (``get_transform('rgb')``, no normalisation), H and W
    multiples of 64 in 64..``max_size`` -> [B,out_channels,H,W] fp32 on the caller's stream.  Batches beyond ``max_batch``
    are chunked.

    ``dtype`` 'fp16' (default) or 'bf16'.  Raw convolution outputs are stored in 16 bit before normalisation, so fp16 can
    overflow on unseen weights: the engine's GroupNorm statistics raise a device flag, which is read after the first forward
    of a set of weights and every ``range_check_every``-th one afterwards; when it is set on finite input the model warns once
    and rebuilds in bf16 (``overflow_fallback=False`` keeps the dtype)."""

    range_check_every = 16

    def __init__(self, downsample: int = 6, in_channels: int = 3, out_channels: int = 3, patch_size: int = 1, dtype: str = "fp16",
                 max_batch: int = 32, max_size: int = 512, init_seed: int = 0, overflow_fallback: bool = True):
        super().__init__()
        if downsample != 6 or in_channels != 3:
            raise NotImplementedError("only downsample=6, in_channels=3 (the published v1 configuration) is supported")
        if not 1 <= out_channels <= 4:
            raise ValueError("out_channels must be in 1..4")
        if dtype not in ("fp16", "bf16"):
            raise ValueError("dtype must be 'fp16' or 'bf16'")
        if max_size % 64 or not 64 <= max_size <= 512:
            raise ValueError("max_size must be a multiple of 64 in 64..512")
        self.downsample, self.in_channels, self.out_channels, self.patch_size = downsample, in_channels, out_channels, patch_size
        self.engine_dtype = dtype
        self.max_batch = max(1, min(int(max_batch), 32))
        self.max_size = int(max_size)
        self.overflow_fallback = bool(overflow_fallback)
        init = unet_init_state_dict(init_seed, out_channels)
        for key in unet_state_dict_spec(out_channels):
            *mods, leaf = key.split(".")
            node = self
            for m in mods:
                if not hasattr(node, m):
                    node.add_module(m, _Node())
                node = getattr(node, m)
            node.register_parameter(leaf, nn.Parameter(init[key], requires_grad=False))
        self._engine: Optional[UNetEngine] = None
        self._engine_key = None
        self._weights_version = 0
        self._range_checked = None
        self._since_range_check = 0

    # ---- keep the engine in sync with the parameters
    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        r = super().load_state_dict(strip_checkpoint(state_dict), strict=strict, **kw)
        self._weights_version += 1
        return r

    def _apply(self, fn, *a, **kw):
        r = super()._apply(fn, *a, **kw)
        self._weights_version += 1
        return r

    @property
    def engine(self) -> Optional[UNetEngine]:
        return self._engine

    def _get_engine(self, device: torch.device) -> UNetEngine:
        index = device.index if device.index is not None else torch.cuda.current_device()
        key = (index, self._weights_version, self.engine_dtype)
        if self._engine is None or self._engine_key != key:
            if self._engine is not None:
                torch.cuda.synchronize(index)
                self._engine.close()
            eng = UNetEngine(self.out_channels, self.max_batch, self.engine_dtype, index, (self.max_size, self.max_size))
            eng.load_state_dict(super().state_dict())
            self._engine, self._engine_key = eng, key
        return self._engine

    def _range_fallback_needed(self, eng: UNetEngine, x: torch.Tensor) -> bool:
        if not (self.overflow_fallback and self.engine_dtype == "fp16"):
            return False
        tag = (self._weights_version, self.engine_dtype)
        first = self._range_checked != tag
        self._since_range_check += 1
        if not first and self._since_range_check < self.range_check_every:
            return False
        self._since_range_check = 0
        if not eng.range_overflowed(reset=True):
            self._range_checked = tag
            return False
        if not bool(torch.isfinite(x).all()):
            return False   # the input's problem, not the arithmetic's
        import warnings
        warnings.warn("omnidata_amd: UNet dtype='fp16' produced non-finite activations -- a convolution output exceeds the fp16 "
                      "range (65504) with these weights; switching this model to dtype='bf16' (fp32's range) and recomputing "
                      "this batch.  Pass overflow_fallback=False to keep the dtype.")
        self.engine_dtype = "bf16"
        return True

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise RuntimeError("omnidata_amd.UNet runs only on an AMD GPU (HIP); got a CPU tensor. There is no CPU fallback -- "
                               "use the reference implementation on CPU.")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 64 or x.shape[3] % 64 or not 64 <= x.shape[2] <= self.max_size \
                or not 64 <= x.shape[3] <= self.max_size:
            raise ValueError(f"expected [B,3,H,W] with H, W multiples of 64 in 64..{self.max_size}, got {tuple(x.shape)}")
        eng = self._get_engine(x.device)
        B, _, H, W = x.shape
        y = torch.empty(B, self.out_channels, H, W, dtype=torch.float32, device=x.device)
        for i in range(0, B, self.max_batch):
            eng.forward(x[i:i + self.max_batch], out=y[i:i + self.max_batch])
        if self._range_fallback_needed(eng, x):
            return self.forward(x)
        return y


def build_unet(task: str = "normal", weights: Optional[str] = None, random_weights: Optional[int] = None, **kw) -> UNet:
    """normal -> 3 channels, depth -> 1 channel (paper_code/test_depth.py:83)."""
    if task not in ("normal", "depth"):
        raise ValueError("task should be one of the following: normal, depth")
    model = UNet(out_channels=3 if task == "normal" else 1, init_seed=0 if random_weights is None else random_weights, **kw)
    if weights is not None:
        model.load_state_dict(torch.load(weights, map_location="cpu", weights_only=False))
    return model.eval()
