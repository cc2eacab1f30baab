"""Ragged-batch pre/post-processing on the GPU (csrc/prepost_batch.hip) against the reference's host path (Pillow / torch):
the uint8 resize and the colormap look-up are integer work and must be bit-exact, for every image of a batch of different
sizes, whatever else is in the batch.  pytest -m gpu."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from omnidata_amd import preprocess as pp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (H, W, mode).  S = 64: tile edges, upscaling, scale 10 (16-row tiles), the scale limit 32 (8-row tiles), both orientations
SMALL = [(70, 90, "RGB"), (64, 64, "L"), (65, 129, "RGB"), (33, 50, "RGB"), (64, 300, "L"), (640, 2048, "RGB"),
         (2048, 64 * 32, "RGB"), (90, 71, "RGB"),
         # the tile height switches from 16 to 8 rows where 17 * scale + 2 exceeds 304 input rows: one image on each side
         (64 * 17, 64 * 17 + 40, "RGB"), (64 * 18, 64 * 18 + 40, "L")]
LARGE = [(512, 640, "RGB"), (385, 777, "RGB"), (384, 384, "RGB"), (400, 400, "L"), (2160, 3840, "RGB")]


def _image(h, w, mode, seed=0):
    rng = np.random.default_rng(1000 * h + w + seed)
    return Image.fromarray(rng.integers(0, 256, (h, w, 3) if mode == "RGB" else (h, w), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def _images(which):
    return tuple(_image(*s) for s in (SMALL if which == "small" else LARGE))


@functools.lru_cache(maxsize=None)
def _reference(which, task):
    """Pillow's result for every image of the set, computed once."""
    S = 64 if which == "small" else 384
    return tuple(pp.image_to_input(img, task, S) for img in _images(which))


@functools.lru_cache(maxsize=None)
def _batched(which, task):
    S = 64 if which == "small" else 384
    return pp.images_to_input_gpu(_images(which), task, S, DEV).cpu()


def _lib():
    from omnidata_amd.engine import load_library
    return load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("in_size,out_size", [(64, 64), (65, 64), (129, 64), (33, 64), (640, 64), (2048, 64), (2047, 64), (1000, 384),
                                              (3840, 614), (12288, 384)])
def test_device_coefficients_equal_the_host_tables(in_size, out_size):
    lib = _lib()
    cap = out_size * 70
    hb, hk, hks = (C.c_int32 * (2 * out_size))(), (C.c_int32 * cap)(), C.c_int32()
    assert lib.dptx_resample_coeffs(in_size, out_size, hb, hk, cap, C.byref(hks)) == 0
    db = torch.full((out_size, 2), -7, dtype=torch.int32, device=DEV)
    dk = torch.full((cap,), -7, dtype=torch.int32, device=DEV)
    dks = C.c_int32()
    assert lib.dptx_resample_coeffs_device(in_size, out_size, db.data_ptr(), dk.data_ptr(), cap, C.byref(dks), _stream()) == 0
    assert dks.value == hks.value
    n = out_size * hks.value
    assert np.array_equal(db.cpu().numpy().reshape(-1), np.frombuffer(hb, dtype=np.int32))
    assert np.array_equal(dk.cpu().numpy()[:n], np.frombuffer(hk, dtype=np.int32)[:n])
    assert bool((dk[n:] == -7).all())


@pytest.mark.parametrize("task", ["normal", "depth"])
@pytest.mark.parametrize("which", ["small", "large"])
def test_ragged_batch_bit_exact_vs_pil_path(which, task):
    got, ref = _batched(which, task), _reference(which, task)
    S = 64 if which == "small" else 384
    assert got.shape == (len(ref), 3, S, S)
    for i, r in enumerate(ref):
        assert torch.equal(got[i:i + 1], r), (which, task, i)


def test_each_image_alone_equals_its_slice_of_the_batch():
    got = _batched("small", "normal")
    for i, img in enumerate(_images("small")):
        assert torch.equal(pp.images_to_input_gpu([img], "normal", 64, DEV).cpu()[0], got[i]), i


def test_reversed_batch_gives_the_reversed_result():
    got = _batched("small", "depth")
    rev = pp.images_to_input_gpu(_images("small")[::-1], "depth", 64, DEV).cpu()
    assert torch.equal(rev.flip(0), got)


def test_batch_of_33_crosses_a_descriptor_chunk():
    imgs = _images("small")[:5]
    alone = _batched("small", "normal")[:5]
    got = pp.images_to_input_gpu([imgs[i % 5] for i in range(33)], "normal", 64, DEV).cpu()
    for i in range(33):
        assert torch.equal(got[i], alone[i % 5]), i


@pytest.mark.parametrize("task", ["normal", "depth"])
def test_batch_equals_the_single_image_entry(task):
    got = _batched("large", task)
    for i, img in enumerate(_images("large")):
        assert torch.equal(pp.image_to_input_gpu(img, task, DEV).cpu()[0], got[i]), i


def test_other_modes_take_the_pil_path_into_their_slot():
    rng = np.random.default_rng(5)
    rgba = Image.fromarray(rng.integers(0, 256, (80, 100, 4), dtype=np.uint8), "RGBA")
    imgs = [_images("small")[0], rgba, _images("small")[2]]
    got = pp.images_to_input_gpu(imgs, "normal", 64, DEV).cpu()
    ref = _reference("small", "normal")
    assert torch.equal(got[0:1], ref[0]) and torch.equal(got[2:3], ref[2])
    assert torch.equal(got[1:2], pp.image_to_input(rgba, "normal", 64))


def _raw_call(arrays, strides, S, task, x):
    """dptx_preprocess_u8_batch on pixel rows `strides[i]` bytes apart (>= W*C: the gap is filled with 0xFF)."""
    from omnidata_amd._native import workspace
    descs = (pp.ImageDesc * len(arrays))()
    chunks, off = [], 0
    for i, (a, st) in enumerate(zip(arrays, strides)):
        H, W, Cn = a.shape
        rows = np.full((H, st), 255, dtype=np.uint8)
        rows[:, :W * Cn] = a.reshape(H, W * Cn)
        descs[i] = pp.ImageDesc(off, H, W, Cn, st)
        pad = (-rows.size) % 16 + 16 * (i % 2)      # offsets that are multiples of 16 and some that are odd
        if i % 2:
            pad += 1
        chunks += [rows.reshape(-1), np.full(pad, 255, dtype=np.uint8)]
        off += rows.size + pad
    dev = torch.from_numpy(np.concatenate(chunks)).to(DEV)
    ws = workspace("dptx_preprocess_batch_workspace_bytes", torch.device(DEV), (len(arrays), S), "unsupported")
    rc = _lib().dptx_preprocess_u8_batch(dev.data_ptr(), C.addressof(descs), len(arrays), S, int(task == "depth"), x.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _stream())
    torch.cuda.synchronize()
    return rc


def test_output_is_covered_guard_untouched_and_padded_rows_give_the_same_bits():
    imgs = _images("small")[:6]
    arrays = [pp._as_hwc_u8(im) for im in imgs]
    B, S, guard = len(arrays), 64, 4096
    n = B * 3 * S * S
    flat = torch.full((n + guard,), float("nan"), device=DEV)
    tight = [a.shape[1] * a.shape[2] for a in arrays]
    assert _raw_call(arrays, tight, S, "normal", flat) == 0
    out = flat.cpu()
    assert not torch.isnan(out[:n]).any()
    assert torch.isnan(out[n:]).all()
    ref = _reference("small", "normal")
    got = out[:n].reshape(B, 3, S, S)
    for i in range(B):
        assert torch.equal(got[i:i + 1], ref[i]), i        # unaligned image offsets included
    flat2 = torch.full((n + guard,), float("nan"), device=DEV)
    padded = [t + p for t, p in zip(tight, (1, 3, 64, 7, 13, 2))]
    assert _raw_call(arrays, padded, S, "normal", flat2) == 0
    assert torch.equal(flat2.cpu()[:n], out[:n]) and torch.isnan(flat2.cpu()[n:]).all()


def test_normal_batch_equals_to_pil_image_per_image():
    y = (torch.rand(3, 3, 64, 64) * 1.4 - 0.2).to(DEV)
    got = pp.normals_to_u8_gpu(y).cpu().numpy()
    assert got.shape == (3, 64, 64, 3)
    for i in range(3):
        assert np.array_equal(got[i], np.asarray(pp.normal_to_pil(y[i].cpu()))), i
    y384 = (torch.rand(2, 3, 384, 384) * 1.4 - 0.2).to(DEV)
    got = pp.normals_to_u8_gpu(y384).cpu()
    for i in range(2):
        assert torch.equal(got[i], pp.normal_to_u8_gpu(y384[i]).cpu()), i


def test_depth_batch_equals_the_single_entry_and_aten_bicubic():
    d = (torch.rand(3, 384, 384) * 1.2 - 0.1).clamp(0, 1).to(DEV)
    got = pp.depths_to_512_gpu(d)
    assert got.shape == (3, 512, 512)
    for i in range(3):
        assert torch.equal(got[i], pp.depth_to_512_gpu(d[i])), i
    ref = 1 - F.interpolate(d.cpu()[:, None], (512, 512), mode="bicubic").clamp(0, 1)[:, 0]
    assert (got.cpu() - ref).abs().max() < 2e-6


def test_colorize_equals_colorize_viridis_on_the_gpus_own_maps():
    d = (torch.rand(4, 384, 384) * 1.2 - 0.1).clamp(0, 1)
    maps = pp.depths_to_512_gpu(d.to(DEV))
    maps[1] = 0.75                            # a constant map: hi == lo
    maps[2, 311, 17] = 1.5                    # a maximum that occurs exactly once
    assert int((maps[2] == maps[2].max()).sum()) == 1 and float(maps[1].min()) == float(maps[1].max())
    got = pp.depths_to_rgba_gpu(maps).cpu().numpy()
    assert got.shape == (4, 512, 512, 4) and got.dtype == np.uint8
    host = maps.cpu().numpy()
    for i in range(4):
        assert np.array_equal(got[i], pp.colorize_viridis(host[i])), i
    # odd sizes, more than one partial block, a non-finite value: every index stays inside the table
    odd = torch.randn(2, 37, 1001, device=DEV)
    got = pp.depths_to_rgba_gpu(odd).cpu().numpy()
    for i in range(2):
        assert np.array_equal(got[i], pp.colorize_viridis(odd[i].cpu().numpy())), i
    odd[0, 3, 5] = float("nan")
    odd[1, 0, 0] = float("inf")
    lut = {tuple(r) for r in pp.viridis_lut().tolist()}
    got = pp.depths_to_rgba_gpu(odd).cpu().numpy().reshape(-1, 4)
    assert {tuple(r) for r in np.unique(got, axis=0).tolist()} <= lut


def test_pre_and_post_entry_points_replay_from_one_captured_graph():
    """No hidden allocation or synchronisation: the calls capture into one (linear) graph, and a replay gives the same bits."""
    from omnidata_amd._native import workspace
    imgs = _images("small")[:4]
    S, B = 64, 4
    buf, descs = pp.pack_images(imgs)
    dev = buf.to(DEV)
    device = torch.device(DEV)
    ws = workspace("dptx_preprocess_batch_workspace_bytes", device, (B, S), "unsupported")
    cws = workspace("dptx_colorize_workspace_bytes", device, (B, 512 * 512), "unsupported")
    lut = torch.from_numpy(pp.viridis_lut()).to(DEV)
    x = torch.zeros(B, 3, S, S, device=DEV)
    u8 = torch.zeros(B, S, S, 3, dtype=torch.uint8, device=DEV)
    d512 = torch.zeros(B, 512, 512, device=DEV)
    rgba = torch.zeros(B, 512, 512, 4, dtype=torch.uint8, device=DEV)
    lib = _lib()

    def run(stream):
        assert lib.dptx_preprocess_u8_batch(dev.data_ptr(), C.addressof(descs), B, S, 0, x.data_ptr(), ws.data_ptr(), ws.numel(),
                                            stream) == 0
        assert lib.dptx_postprocess_normal_u8_batch(x.data_ptr(), B, S, u8.data_ptr(), stream) == 0
        assert lib.dptx_postprocess_depth_batch(x.data_ptr(), B, S, d512.data_ptr(), stream) == 0   # channel planes as maps
        assert lib.dptx_colorize_u8_batch(d512.data_ptr(), lut.data_ptr(), B, 512 * 512, rgba.data_ptr(), cws.data_ptr(),
                                          cws.numel(), stream) == 0

    run(_stream())
    torch.cuda.synchronize()
    want = [t.clone() for t in (x, u8, d512, rgba)]
    assert torch.equal(x.cpu(), _batched("small", "normal")[:4])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(_stream())
    for t in (x, u8, d512, rgba):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for t, w in zip((x, u8, d512, rgba), want):
        assert torch.equal(t, w)
