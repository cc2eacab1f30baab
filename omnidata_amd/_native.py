"""What the wrappers of libdptx's feature entry points (refocus.py, midas_loss.py, virtual_normal_loss.py, normal_loss.py) share: the
CUDA-tensor check, the cached workspace and the checked call (the current stream is engine._stream); and what the inference layer
(preprocess.py) adds to them: the descriptor chunks of a batched entry point and the colormap table on the device."""
from __future__ import annotations

import ctypes as C

import torch

from .engine import load_library

_ws_cache: dict = {}
_lut_cache: dict = {}
MAX_DESCS = 4096     # include/dptx.h: descriptors per call of a batched entry point


def check_cuda(name: str, t) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA tensor (omnidata_amd has no CPU path)")


def call(name: str, *args) -> None:
    """load_library().<name>(*args); a non-zero return code raises RuntimeError."""
    rc = getattr(load_library(), name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc})")


def workspace(name: str, device, shape: tuple, unsupported: str) -> torch.Tensor:
    """The uint8 workspace tensor of the size <name>(*shape, &bytes) asks for, one per (name, device, shape), kept for the
    life of the process; ValueError(unsupported) where the entry point rejects the shape."""
    nbytes = C.c_int64()
    if getattr(load_library(), name)(*shape, C.byref(nbytes)) != 0:
        raise ValueError(unsupported)
    key = (name, str(device), *shape)
    ws = _ws_cache.get(key)
    if ws is None:
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def chunks(n: int, step: int = MAX_DESCS):
    """Yields (b0, count): one entry-point call per `step` descriptors."""
    for b0 in range(0, n, step):
        yield b0, min(step, n - b0)


def at(array, b0: int) -> int:
    """The address of element b0 of a ctypes array."""
    return C.addressof(array) + b0 * C.sizeof(array._type_)


def viridis_lut_on(device) -> torch.Tensor:
    """preprocess.viridis_lut() as a [256,4] uint8 tensor on `device`, one per device, kept for the life of the process."""
    lut = _lut_cache.get(str(device))
    if lut is None:
        from .preprocess import viridis_lut
        lut = _lut_cache[str(device)] = torch.from_numpy(viridis_lut()).to(device)
    return lut
