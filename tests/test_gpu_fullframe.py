"""Full-frame inference on the GPU (csrc/fullframe.hip, omnidata_amd/batch_infer.py): the rectangular ragged-batch resize against
Pillow (bit-exact), the ragged outputs against ATen's F.interpolate on the CPU, and the pipeline end to end.  pytest -m gpu.

Measured on an MI355X (the ratios of (c) are in profiles/fullframe_parity.md)."""
import ctypes as C
import functools
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from omnidata_amd import preprocess as pp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMAL_U8, NORMAL_F32, DEPTH_F32, DEPTH_RGBA, RENORM = 1, 2, 3, 4, 16

# ------------------------------------------------------------------------------------------------ pre
# (H, W, mode): up on both axes, tile edges, strong down, 32x down on one axis and up on the other (against (64, 96))
IMAGES = [(33, 50, "RGB"), (70, 90, "RGB"), (64, 64, "L"), (65, 129, "RGB"), (640, 2048, "RGB"), (2048, 64, "RGB"), (90, 71, "RGB")]
TARGETS = [(64, 96), (96, 64), (384, 512)]


def _image(h, w, mode, seed=0):
    rng = np.random.default_rng(1000 * h + w + seed)
    return Image.fromarray(rng.integers(0, 256, (h, w, 3) if mode == "RGB" else (h, w), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def _images():
    return tuple(_image(*s) for s in IMAGES)


def _pil_reference(img, task, net):
    OH, OW = net
    t = pp.to_tensor(img.resize((OW, OH), Image.BILINEAR))
    if task == "depth":
        t = (t - 0.5) / 0.5                      # Normalize(0.5, 0.5)
    if t.shape[0] == 1:
        t = t.repeat_interleave(3, 0)
    return t


@functools.lru_cache(maxsize=None)
def _reference(task, net):
    return tuple(_pil_reference(img, task, net) for img in _images())


@functools.lru_cache(maxsize=None)
def _batched(task, net):
    return pp.images_to_input_rect_gpu(_images(), task, net, DEV).cpu()


def _lib():
    from omnidata_amd.engine import load_library
    return load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("task", ["normal", "depth"])
@pytest.mark.parametrize("net", TARGETS)
def test_rect_batch_bit_exact_vs_pillow(net, task):
    got, ref = _batched(task, net), _reference(task, net)
    assert got.shape == (len(ref), 3, *net)
    for i, r in enumerate(ref):
        assert torch.equal(got[i], r), (net, task, IMAGES[i])


def test_each_image_alone_equals_its_slice_of_the_batch():
    got = _batched("normal", (64, 96))
    for i, img in enumerate(_images()):
        assert torch.equal(pp.images_to_input_rect_gpu([img], "normal", (64, 96), DEV).cpu()[0], got[i]), i


def test_reversed_batch_gives_the_reversed_result():
    rev = pp.images_to_input_rect_gpu(_images()[::-1], "depth", (96, 64), DEV).cpu()
    assert torch.equal(rev.flip(0), _batched("depth", (96, 64)))


def test_batch_of_33_crosses_a_descriptor_chunk():
    imgs, alone = _images(), _batched("normal", (64, 96))
    got = pp.images_to_input_rect_gpu([imgs[i % 7] for i in range(33)], "normal", (64, 96), DEV).cpu()
    for i in range(33):
        assert torch.equal(got[i], alone[i % 7]), i


def test_other_modes_take_the_pil_path_into_their_slot():
    rng = np.random.default_rng(5)
    rgba = Image.fromarray(rng.integers(0, 256, (80, 100, 4), dtype=np.uint8), "RGBA")
    imgs = [_images()[0], rgba, _images()[2]]
    got = pp.images_to_input_rect_gpu(imgs, "normal", (64, 96), DEV).cpu()
    ref = _reference("normal", (64, 96))
    assert torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2])
    assert torch.equal(got[1], pp.to_tensor(rgba.resize((96, 64), Image.BILINEAR))[:3])


def test_padded_rows_unaligned_offsets_and_the_guard_behind_the_output():
    """Pixel rows `stride` bytes apart (the gap holds 0xFF), images at odd offsets: the same bits, and nothing behind x."""
    from omnidata_amd._native import workspace
    arrays = [pp._as_hwc_u8(im) for im in _images()[:4]]
    OH, OW, B, guard = 64, 96, 4, 4096
    descs = (pp.ImageDesc * B)()
    chunks, off = [], 0
    for i, (a, extra) in enumerate(zip(arrays, (1, 3, 64, 7))):
        H, W, Cn = a.shape
        rows = np.full((H, W * Cn + extra), 255, dtype=np.uint8)
        rows[:, :W * Cn] = a.reshape(H, W * Cn)
        descs[i] = pp.ImageDesc(off, H, W, Cn, W * Cn + extra)
        pad = (-rows.size) % 16 + (i % 2)
        chunks += [rows.reshape(-1), np.full(pad, 255, dtype=np.uint8)]
        off += rows.size + pad
    dev = torch.from_numpy(np.concatenate(chunks)).to(DEV)
    n = B * 3 * OH * OW
    flat = torch.full((n + guard,), float("nan"), device=DEV)
    ws = workspace("dptx_preprocess_rect_batch_workspace_bytes", torch.device(DEV), (B, OH, OW), "unsupported")
    assert _lib().dptx_preprocess_u8_rect_batch(dev.data_ptr(), C.addressof(descs), B, OH, OW, 0, flat.data_ptr(), ws.data_ptr(),
                                                ws.numel(), _stream()) == 0
    out = flat.cpu()
    assert torch.isnan(out[n:]).all()
    assert torch.equal(out[:n].reshape(B, 3, OH, OW), _batched("normal", (OH, OW))[:4])


# ------------------------------------------------------------------------------------------------ post
h0, w0 = 64, 96
SIZES = [(64, 96), (128, 192), (37, 1001), (50, 70), (1, 1), (129, 193)]
BOUND_ABS = 2e-6            # the project's bound for this op (tests/test_gpu_prepost.py)


@functools.lru_cache(maxsize=None)
def _source(Cn):
    """[3, C, 64, 96] in [-0.2, 1.2]; output i of SIZES reads map i % 3."""
    g = torch.Generator().manual_seed(7 + Cn)
    return torch.rand(3, Cn, h0, w0, generator=g) * 1.4 - 0.2


def _six(Cn):
    return _source(Cn)[[i % 3 for i in range(len(SIZES))]].contiguous()


def _aten(y, size, kind, dtype, renorm=False):
    """The reference on the CPU: F.interpolate, then what the mode does with it."""
    v = F.interpolate(y.to(dtype)[None], size, mode="bilinear" if kind == "normal" else "bicubic", align_corners=False)[0]
    if kind == "depth":
        return 1 - v.clamp(0, 1)[0]
    if renorm:
        v = (F.normalize(2 * v - 1, dim=0) + 1) / 2
    return v.clamp(0, 1)


@functools.lru_cache(maxsize=None)
def _got(mode, renorm=False):
    Cn = 3 if mode.startswith("normal") else 1
    return tuple(t.cpu() for t in pp.resize_outputs_gpu(_six(Cn).to(DEV), SIZES, mode, renorm))


def _quant(v):
    return v.mul(255).to(torch.uint8)        # ToPILImage: mul(255).byte() truncates


def test_identity_size_is_the_plain_clamp_and_quantise_of_the_source():
    n, d = _six(3)[0], _six(1)[0, 0]
    assert torch.equal(_got("normal_f32")[0], n.clamp(0, 1))
    assert torch.equal(_got("normal_u8")[0], _quant(n.clamp(0, 1)).permute(1, 2, 0))
    assert torch.equal(_got("depth_f32")[0], 1 - d.clamp(0, 1))


@pytest.mark.parametrize("factor", [2, 4])
def test_exact_case_bilinear_equals_aten_bit_for_bit(factor):
    """Source on multiples of 2^-8, x2 and x4: every weight and product is exact in fp32, so there is one right answer."""
    y = (_source(3) * 256).round() / 256
    size = (h0 * factor, w0 * factor)
    ref = [_aten(y[i], size, "normal", torch.float32) for i in range(3)]
    for i in range(3):
        assert torch.equal(ref[i].double(), _aten(y[i], size, "normal", torch.float64))     # ATen fp32 == ATen fp64
    got = pp.resize_outputs_gpu(y.to(DEV), [size] * 3, "normal_f32")
    u8 = pp.resize_outputs_gpu(y.to(DEV), [size] * 3, "normal_u8")
    for i in range(3):
        assert torch.equal(got[i].cpu(), ref[i]), i
        assert torch.equal(u8[i].cpu(), _quant(ref[i]).permute(1, 2, 0)), i


@pytest.mark.parametrize("mode,renorm", [("normal_f32", False), ("normal_f32", True), ("depth_f32", False)])
def test_general_sizes_within_twice_the_references_own_rounding(mode, renorm):
    """e_ref = max|ATen fp32 - ATen fp64| on the CPU is the reference's own coordinate-rounding error for the case; required:
    max|got - ATen fp64| <= 2 * e_ref + 2e-6 (a different blend order on top of the same coordinate rounding; a wrong tap is
    >= 1e-2)."""
    kind = "normal" if mode.startswith("normal") else "depth"
    y = _six(3 if kind == "normal" else 1)
    got = _got(mode, renorm)
    for i, size in enumerate(SIZES):
        r64 = _aten(y[i], size, kind, torch.float64, renorm)
        e_ref = float((_aten(y[i], size, kind, torch.float32, renorm).double() - r64).abs().max())
        err = float((got[i].double() - r64).abs().max())
        print(f"parity {mode}{'+renorm' if renorm else ''} {size}: e_ref {e_ref:.3e} err {err:.3e} "
              f"err / (2 e_ref + 2e-6) = {err / (2 * e_ref + BOUND_ABS):.3f}")
        assert got[i].shape == r64.shape
        assert err <= 2 * e_ref + BOUND_ABS, (mode, renorm, size, err, e_ref)


def test_renormalised_normals_have_unit_length():
    for t in _got("normal_f32", True):
        n = 2 * t.double() - 1
        assert float((n.pow(2).sum(0).sqrt() - 1).abs().max()) <= 1e-6


@pytest.mark.parametrize("renorm", [False, True])
def test_uint8_is_the_truncation_of_the_entrys_own_fp32_and_within_one_level_of_aten(renorm):
    y = _six(3)
    for i, (u8, f32) in enumerate(zip(_got("normal_u8", renorm), _got("normal_f32", renorm))):
        assert u8.shape == (*SIZES[i], 3) and u8.dtype == torch.uint8
        assert torch.equal(u8, _quant(f32).permute(1, 2, 0)), i
        ref = _quant(_aten(y[i], SIZES[i], "normal", torch.float32, renorm)).permute(1, 2, 0)
        assert int((u8.int() - ref.int()).abs().max()) <= 1, i


def test_depth_rgba_is_colorize_viridis_of_the_entrys_own_depth_maps():
    for i, (rgba, f32) in enumerate(zip(_got("depth_rgba"), _got("depth_f32"))):
        assert rgba.shape == (*SIZES[i], 4) and rgba.dtype == torch.uint8
        assert np.array_equal(rgba.numpy(), pp.colorize_viridis(f32.numpy())), i


def _raw_post(y, sizes, code, guard=64):
    """dptx_postprocess_resize_batch into a buffer of 0xA5 with padded rows and gaps between the outputs -> (buffer, mask of the
    bytes the outputs own, per-output extraction)."""
    from omnidata_amd._native import workspace
    u8 = (code & 15) == NORMAL_U8
    bpp, planes = (3 if u8 else 4), (3 if (code & 15) == NORMAL_F32 else 1)
    descs = (pp.ImageDesc * len(sizes))()
    off, spans = (1 if u8 else 4), []
    for i, (H, W) in enumerate(sizes):
        stride = W * bpp + ((1, 2, 3, 5)[i % 4] if u8 else 4 * (1 + i % 3))
        descs[i] = pp.ImageDesc(off, H, W, 3, stride)
        spans.append((off, planes * H, W * bpp, stride))
        off += planes * H * stride + ((3, 1, 6)[i % 3] if u8 else 8)
    buf = torch.full((off + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    lut = torch.from_numpy(pp.viridis_lut()).to(DEV)
    ws = workspace("dptx_postprocess_resize_workspace_bytes", torch.device(DEV), (len(sizes), DEPTH_RGBA), "unsupported")
    assert _lib().dptx_postprocess_resize_batch(y.data_ptr(), len(sizes), y.shape[1], y.shape[2], y.shape[3], C.addressof(descs), code,
                                                buf.data_ptr(), lut.data_ptr(), ws.data_ptr(), ws.numel(), _stream()) == 0
    host = buf.cpu().numpy()
    owned = np.zeros(host.shape, dtype=bool)
    outs = []
    for o, rows, rowbytes, stride in spans:
        idx = o + np.arange(rows)[:, None] * stride + np.arange(rowbytes)[None, :]
        owned[idx] = True
        outs.append(host[idx])
    return host, owned, outs


@pytest.mark.parametrize("mode,code", [("normal_u8", NORMAL_U8), ("normal_u8", NORMAL_U8 | RENORM), ("normal_f32", NORMAL_F32),
                                       ("depth_f32", DEPTH_F32), ("depth_rgba", DEPTH_RGBA)])
def test_guard_bytes_between_after_and_in_row_padding_are_untouched(mode, code):
    """W = 1001 and W = 37: 3 * W is no multiple of 4, rows start at every byte alignment."""
    sizes = SIZES + [(5, 37), (3, 129)]
    Cn = 3 if mode.startswith("normal") else 1
    y = _source(Cn)[[i % 3 for i in range(len(sizes))]].contiguous()
    host, owned, outs = _raw_post(y.to(DEV), sizes, code)
    assert (host[~owned] == 0xA5).all()
    tight = pp.resize_outputs_gpu(y.to(DEV), sizes, mode, bool(code & RENORM))
    for i, (o, t) in enumerate(zip(outs, tight)):
        assert np.array_equal(o.reshape(-1), t.cpu().contiguous().view(torch.uint8).numpy().reshape(-1)), i   # padded == tight


@pytest.mark.parametrize("mode", ["normal_u8", "depth_rgba"])
def test_each_output_alone_equals_its_slot_of_the_batch_and_33_cross_a_chunk(mode):
    Cn = 3 if mode.startswith("normal") else 1
    y = _six(Cn).to(DEV)
    got = _got(mode)
    for i, size in enumerate(SIZES):
        assert torch.equal(pp.resize_outputs_gpu(y[i:i + 1], [size], mode)[0].cpu(), got[i]), i
    many = pp.resize_outputs_gpu(y[[i % 6 for i in range(33)]].contiguous(), [SIZES[i % 6] for i in range(33)], mode)
    for i in range(33):
        assert torch.equal(many[i].cpu(), got[i % 6]), i


def test_pre_and_post_entry_points_replay_from_one_captured_graph():
    """No hidden allocation or synchronisation: the calls capture into one (linear) graph, and a replay gives the same bits."""
    from omnidata_amd._native import workspace
    imgs = _images()[:4]
    OH, OW, B = 64, 96, 4
    buf, descs = pp.pack_images(imgs)
    dev = buf.to(DEV)
    device = torch.device(DEV)
    ws = workspace("dptx_preprocess_rect_batch_workspace_bytes", device, (B, OH, OW), "unsupported")
    pws = workspace("dptx_postprocess_resize_workspace_bytes", device, (B, DEPTH_RGBA), "unsupported")
    lut = torch.from_numpy(pp.viridis_lut()).to(DEV)
    sizes = [(im.size[1], im.size[0]) for im in imgs]
    nd, n_total = pp.output_layout(sizes, "normal_u8")
    dd, d_total = pp.output_layout(sizes, "depth_rgba")
    x = torch.zeros(B, 3, OH, OW, device=DEV)
    u8 = torch.zeros(n_total, dtype=torch.uint8, device=DEV)
    rgba = torch.zeros(d_total, dtype=torch.uint8, device=DEV)
    lib = _lib()

    def run(stream):
        assert lib.dptx_preprocess_u8_rect_batch(dev.data_ptr(), C.addressof(descs), B, OH, OW, 0, x.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), stream) == 0
        assert lib.dptx_postprocess_resize_batch(x.data_ptr(), B, 3, OH, OW, C.addressof(nd), NORMAL_U8 | RENORM, u8.data_ptr(), None,
                                                 None, 0, stream) == 0
        # the first B channel planes of x read as depth maps [B][1][OH][OW]
        assert lib.dptx_postprocess_resize_batch(x.data_ptr(), B, 1, OH, OW, C.addressof(dd), DEPTH_RGBA, rgba.data_ptr(),
                                                 lut.data_ptr(), pws.data_ptr(), pws.numel(), stream) == 0

    run(_stream())
    torch.cuda.synchronize()
    want = [t.clone() for t in (x, u8, rgba)]
    assert torch.equal(x.cpu(), _batched("normal", (OH, OW))[:4])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(_stream())
    for t in (x, u8, rgba):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for t, w in zip((x, u8, rgba), want):
        assert torch.equal(t, w)
    assert bool(u8.any()) and bool(rgba.any())


# ------------------------------------------------------------------------------------------------ end to end
E2E = [("a", (70, 90)), ("b", (90, 70)), ("c", (64, 64)), ("d", (33, 50)), ("e", (120, 300))]    # (H, W)


def _folder(path, shapes=E2E):
    rng = np.random.default_rng(11)
    path.mkdir()
    for stem, (h, w) in shapes:
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path / f"{stem}.png")
    return [str(path / f"{stem}.png") for stem, _ in shapes]


@functools.lru_cache(maxsize=None)
def _model(task):
    from omnidata_amd.model import build_model
    return build_model(task, random_weights=0, dtype="bf16", max_batch=2).to(DEV)


@pytest.mark.parametrize("task,full_frame,renorm", [("normal", "squash", False), ("normal", "aspect", True), ("depth", "aspect", False)])
def test_files_have_the_inputs_sizes_and_the_pixels_of_the_pieces_called_by_hand(tmp_path, task, full_frame, renorm):
    from omnidata_amd.batch_infer import BatchPredictor
    files = _folder(tmp_path / "in")
    model = _model(task)
    bp = BatchPredictor(model, task, batch_size=2, image_size=64, full_frame=full_frame, renormalize=renorm)
    bp.predict_to_dir(files[::-1], str(tmp_path / "out"))                       # any input order
    assert sorted(os.listdir(tmp_path / "out")) == sorted(f"{s}_{k}.png" for s, _ in E2E for k in (task, "rgb"))
    outs = list(bp.predict(files))
    assert len(outs) == len(files)
    for f, (stem, (h, w)), o in zip(files, E2E, outs):
        img = Image.open(f)
        net = (64, 64) if full_frame == "squash" else pp.full_frame_net_size(w, h, 64)[1::-1]
        x = pp.images_to_input_rect_gpu([img], task, net, DEV)
        y = model(x).clamp(0, 1)
        want = pp.resize_outputs_gpu(y, [(h, w)], "depth_rgba" if task == "depth" else "normal_u8", renorm)[0]
        assert o.is_cuda and o.dtype == torch.uint8 and o.shape == (h, w, 4 if task == "depth" else 3)
        assert torch.equal(o, want), stem                                       # in input order: this file's own result
        png = Image.open(tmp_path / "out" / f"{stem}_{task}.png")
        assert png.size == (w, h) and np.array_equal(np.asarray(png), want.cpu().numpy()), stem
        rgb = Image.open(tmp_path / "out" / f"{stem}_rgb.png")
        assert rgb.size == (w, h) and np.array_equal(np.asarray(rgb), np.asarray(img)), stem


def test_an_unreadable_file_raises_before_anything_has_run_or_is_written(tmp_path):
    """What BatchPredictor._chunks promises for the full-frame paths: the sizes are read from the headers first."""
    from PIL import UnidentifiedImageError
    from omnidata_amd.batch_infer import BatchPredictor
    files = _folder(tmp_path / "in", E2E[:2])
    bad = tmp_path / "in" / "notes.txt"
    bad.write_text("not an image\n")
    out = tmp_path / "out"
    bp = BatchPredictor(_model("normal"), "normal", batch_size=2, image_size=64, full_frame="squash")
    with pytest.raises(UnidentifiedImageError):
        bp.predict_to_dir([files[0], str(bad), files[1]], str(out))
    assert os.listdir(out) == []


def test_without_full_frame_the_predictor_gives_todays_pixels(tmp_path):
    from omnidata_amd.batch_infer import BatchPredictor
    files = _folder(tmp_path / "in", [("a", (400, 520)), ("b", (390, 384))])
    model = _model("normal")
    outs = list(BatchPredictor(model, "normal", batch_size=2).predict(files))
    for f, o in zip(files, outs):
        x = pp.image_to_input(Image.open(f), "normal").to(DEV)
        assert o.shape == (384, 384, 3) and torch.equal(o, pp.normal_to_u8_gpu(model(x).clamp(0, 1)[0])), f


def test_demo_cli_full_frame_aspect_on_a_two_image_folder(tmp_path):
    files = _folder(tmp_path / "in", [("a", (400, 520)), ("b", (390, 300))])
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo.py"), "--task", "normal", "--img_path", str(tmp_path / "in"),
                        "--output_path", str(out), "--random-weights", "0", "--dtype", "bf16", "--full_frame", "aspect", "--renormalize"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    order = glob.glob(str(tmp_path / "in") + "/*")
    lines = [l for l in r.stdout.splitlines() if l.startswith("Reading input")]
    assert lines == [f"Reading input {f} ..." for f in order]                   # reported in input order
    for stem, (h, w) in (("a", (400, 520)), ("b", (390, 300))):
        assert Image.open(out / f"{stem}_normal.png").size == (w, h) and Image.open(out / f"{stem}_rgb.png").size == (w, h)
