"""Test-time augmentation for surface normals on the GPU (csrc/tta.hip, the views entry of csrc/fullframe.hip, omnidata_amd/tta.py):
the view inputs against Pillow (bit-exact), the merge against its restatement (tests/tta_restatement.py), the edges of the
selection, and the pipeline end to end.  pytest -m gpu.

Measured on an MI355X: profiles/tta_parity.md."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

from omnidata_amd import preprocess as pp
from omnidata_amd.tta import five_crops, plan_views
from tta_restatement import merge_restatement, synthetic_view

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMAL_U8, NORMAL_F32 = 1, 2
BOUND_ABS = 2e-6            # the project's bound for a bilinear resize (tests/test_gpu_fullframe.py)


def _lib():
    from omnidata_amd.engine import load_library
    return load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ views
def _two_images():
    rng = np.random.default_rng(61083)
    return (Image.fromarray(rng.integers(0, 256, (61, 83, 3), dtype=np.uint8)),
            Image.fromarray(rng.integers(0, 256, (40, 50), dtype=np.uint8)))


def _windows(img):
    w, h = img.size
    return [(0, 0, w, h)] + five_crops(w, h, 0.8)


@pytest.mark.parametrize("net", [(64, 96), (96, 64)])
def test_views_are_bit_exact_to_pillow_and_unflipped_they_are_the_rect_entry(net):
    from omnidata_amd._native import workspace
    OH, OW = net
    images = _two_images()
    buf, descs = pp.pack_images(images)                              # both images in the same packed buffer, uploaded once
    dev = buf.to(DEV)
    wins, flips, want = [], [], []
    for i, img in enumerate(images):
        for box in _windows(img):
            for flip in (False, True):
                wins.append(pp.window_desc(descs[i], box))
                flips.append(flip)
                view = img.crop(box).resize((OW, OH), Image.BILINEAR)
                t = pp.to_tensor(ImageOps.mirror(view) if flip else view)
                want.append(t.repeat_interleave(3, 0) if t.shape[0] == 1 else t)
    assert len(wins) == 24
    got = pp.views_to_input_gpu(dev, wins, flips, net).cpu()
    for k in range(24):
        assert torch.equal(got[k], want[k]), (net, k, flips[k])
    # flips = NULL: dptx_preprocess_u8_rect_batch on the same descriptors, bit for bit
    plain = pp.views_to_input_gpu(dev, wins, None, net)
    arr = (pp.ImageDesc * 24)(*wins)
    ws = workspace("dptx_preprocess_rect_batch_workspace_bytes", torch.device(DEV), (24, OH, OW), "unsupported")
    rect = torch.full((24, 3, OH, OW), float("nan"), device=DEV)
    assert _lib().dptx_preprocess_u8_rect_batch(dev.data_ptr(), C.addressof(arr), 24, OH, OW, 0, rect.data_ptr(), ws.data_ptr(),
                                                ws.numel(), _stream()) == 0
    assert torch.equal(plain, rect)
    assert torch.equal(plain[0::2].cpu(), got[0::2]) and torch.equal(plain[1::2].flip(-1).cpu(), got[1::2])


# ------------------------------------------------------------------------------------------------ merge against the restatement
SIZE = (70, 93)                                                       # (H, W)
SCALED_OASIS = [(0.8, [192], True), (0.9, [192, 64], True), (1.0, [192, 64, 96, 128, 160], True)]   # "oasis" at 3/8 of its sides


def _windows_of(plan):
    return [(box[1], box[0], box[3] - box[1], box[2] - box[0], int(flip)) for box, flip, _, _ in plan]


@functools.lru_cache(maxsize=None)
def _oasis_case():
    plan = plan_views(SIZE[1], SIZE[0], SCALED_OASIS)
    assert len(plan) == 40
    nets = [net for _, _, _, net in plan]
    assert min(nets) == (64, 96) and max(nets) == (192, 256)
    windows = _windows_of(plan)
    return tuple(synthetic_view(k, *nets[k], windows[k], SIZE) for k in range(40)), tuple(windows)


@functools.lru_cache(maxsize=None)
def _oasis_reference(merger, normalize):
    maps, windows = _oasis_case()
    r64, shortest_view, shortest_merged = merge_restatement(maps, windows, SIZE, merger, normalize, torch.float64, details=True)
    r32 = merge_restatement(maps, windows, SIZE, merger, normalize, torch.float32)
    return r64, float((r32.double() - r64).abs().max()), shortest_view, shortest_merged


def _pack(maps_per_image, windows_per_image):
    """-> (flat fp32 device tensor, [TtaView]): every map back to back, image-major."""
    views, chunks, off = [], [], 0
    for i, (maps, windows) in enumerate(zip(maps_per_image, windows_per_image)):
        for m, (y0, x0, ch, cw, flip) in zip(maps, windows):
            views.append(pp.TtaView(4 * off, m.shape[1], m.shape[2], i, y0, x0, ch, cw, flip))
            chunks.append(m.reshape(-1))
            off += m.numel()
    return torch.cat(chunks).to(DEV), views


def _merge(maps, windows, size, merger="median", normalize=True, output="f32"):
    flat, views = _pack([maps], [windows])
    return pp.merge_normal_views_gpu(flat, views, [size], merger, normalize, output)[0]


@functools.lru_cache(maxsize=None)
def _oasis_got(merger, normalize, output="f32"):
    maps, windows = _oasis_case()
    return _merge(maps, windows, SIZE, merger, normalize, output).cpu()


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("merger", ["median", "mean"])
def test_forty_views_within_twice_the_restatements_own_rounding(merger, normalize):
    """e_ref = max|fp32 restatement - fp64 restatement| is the composition's own rounding for the case; required:
    max|got - fp64 restatement| <= 2 * e_ref + 2e-6 (the criterion of test_general_sizes_within_twice_the_references_own_rounding;
    a wrong tap, a wrong middle element or a missing view is >= 1e-3).  Both divisors of the normalisations stay above 0.25, so
    neither amplifies a rounding difference beyond what e_ref carries."""
    r64, e_ref, shortest_view, shortest_merged = _oasis_reference(merger, normalize)
    got = _oasis_got(merger, normalize)
    err = float((got.double() - r64).abs().max())
    print(f"tta parity {merger}{'' if normalize else '+raw'} {SIZE} 40 views: e_ref {e_ref:.3e} err {err:.3e} "
          f"err / (2 e_ref + 2e-6) = {err / (2 * e_ref + BOUND_ABS):.3f}; shortest view vector {shortest_view:.3f}, "
          f"shortest merged vector {shortest_merged:.3f}")
    assert shortest_view >= 0.25 and shortest_merged >= 0.25
    assert got.shape == r64.shape == (3, *SIZE)
    assert err <= 2 * e_ref + BOUND_ABS, (merger, normalize, err, e_ref)
    n = 2 * got.double() - 1
    assert float((n.pow(2).sum(0).sqrt() - 1).abs().max()) <= 1e-6                        # unit length again


def _raw_merge(flat, views, sizes, code, guard=64):
    """dptx_tta_merge_normals into a buffer of 0xA5 with padded rows, an odd offset and gaps between the outputs -> (buffer,
    mask of the bytes the outputs own, per-output rows)."""
    u8 = (code & 15) == NORMAL_U8
    bpp, planes = (3 if u8 else 4), (1 if u8 else 3)
    descs = (pp.ImageDesc * len(sizes))()
    off, spans = (1 if u8 else 4), []
    for i, (H, W) in enumerate(sizes):
        stride = W * bpp + ((1, 2, 3, 5)[i % 4] if u8 else 4 * (1 + i % 3))
        descs[i] = pp.ImageDesc(off, H, W, 3, stride)
        spans.append((off, planes * H, W * bpp, stride))
        off += planes * H * stride + ((3, 1, 6)[i % 3] if u8 else 8)
    buf = torch.full((off + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    arr = (pp.TtaView * len(views))(*views)
    assert _lib().dptx_tta_merge_normals(flat.data_ptr(), C.addressof(arr), len(views), C.addressof(descs), len(sizes), code,
                                         buf.data_ptr(), _stream()) == 0
    host = buf.cpu().numpy()
    owned = np.zeros(host.shape, dtype=bool)
    outs = []
    for o, rows, rowbytes, stride in spans:
        idx = o + np.arange(rows)[:, None] * stride + np.arange(rowbytes)[None, :]
        owned[idx] = True
        outs.append(host[idx])
    return host, owned, outs


@pytest.mark.parametrize("merger", ["median", "mean"])
def test_uint8_is_the_truncation_of_the_kernels_own_fp32_and_canaries_stay(merger):
    """Padded row strides, an odd output offset (3 * 93 bytes per row: rows start at every byte alignment), 0xA5 around every
    row; a second, narrower image in the same call."""
    maps, windows = _oasis_case()
    small = (9, 13)
    smaps, swins = maps[30:34], [(0, 0, 9, 13, f) for f in (0, 1, 0, 1)]
    flat, views = _pack([maps, smaps], [windows, swins])
    code = pp.TTA_MEAN if merger == "mean" else 0
    f32 = [_oasis_got(merger, True), _merge(smaps, swins, small, merger).cpu()]
    host, owned, outs = _raw_merge(flat, views, [SIZE, small], NORMAL_U8 | code)
    assert (host[~owned] == 0xA5).all()
    for o, f, (H, W) in zip(outs, f32, (SIZE, small)):
        want = f.clamp(0, 1).mul(255).to(torch.uint8).permute(1, 2, 0)                    # ToPILImage: mul(255).byte() truncates
        assert np.array_equal(o.reshape(H, W, 3), want.numpy())
    host, owned, outs = _raw_merge(flat, views, [SIZE, small], NORMAL_F32 | code)
    assert (host[~owned] == 0xA5).all()
    for o, f, (H, W) in zip(outs, f32, (SIZE, small)):
        assert np.array_equal(np.ascontiguousarray(o).view(np.float32).reshape(3, H, W), f.numpy())     # padded == tight
    assert torch.equal(_oasis_got(merger, True, "u8"), f32[0].mul(255).to(torch.uint8).permute(1, 2, 0))


# ------------------------------------------------------------------------------------------------ edges of the selection
EDGE = (9, 13)


@functools.lru_cache(maxsize=None)
def _stacked_views(n):
    """n views of the whole 9 x 13 image (every pixel is covered n times), alternately plain and flipped, maps of 16 x 24."""
    windows = tuple((0, 0, *EDGE, k % 2) for k in range(n))
    return tuple(synthetic_view(100 + k, 16, 24, windows[k], EDGE, noise=0.2) for k in range(n)), windows


@pytest.mark.parametrize("n", [1, 2, 3, 8, 9, 16, 17, 32, 33, 63, 64])
def test_every_count_up_to_64_on_one_pixel_class(n):
    """One view, both sides of every views-per-image class (8 / 16 / 32 / 64), odd and even counts; median and mean."""
    maps, windows = _stacked_views(n)
    for merger in ("median", "mean"):
        r64 = merge_restatement(maps, windows, EDGE, merger, True, torch.float64)
        e_ref = float((merge_restatement(maps, windows, EDGE, merger, True, torch.float32).double() - r64).abs().max())
        err = float((_merge(maps, windows, EDGE, merger).cpu().double() - r64).abs().max())
        print(f"tta parity {merger} {n} stacked views: e_ref {e_ref:.3e} err {err:.3e}")
        assert err <= 2 * e_ref + BOUND_ABS, (n, merger, err, e_ref)


def test_the_views_per_image_class_does_not_change_a_bit():
    """min / max move values and never round them: the same 5 covering views inside sets of 5, 9, 17 and 33 views (the kernel's
    four classes) whose extra views lie in a 14th column give the same bits in the first 13."""
    maps, windows = _stacked_views(33)
    size = (EDGE[0], EDGE[1] + 1)                                                          # a 14th column for the extra views
    want = None
    for n in (5, 9, 17, 33):
        wins = list(windows[:5]) + [(0, EDGE[1], EDGE[0], 1, 0)] * (n - 5)
        got = _merge(maps[:n], wins, size).cpu()[:, :, :EDGE[1]]
        want = got if want is None else want
        assert torch.equal(got, want), n
    assert torch.equal(want, _merge(maps[:5], windows[:5], EDGE).cpu())


def test_two_views_give_their_mean_and_no_view_gives_one_half():
    """Columns 0-4: view a only; 5-8: a and b (the median of two is their mean, bit for bit); 9-10: b only; 11-12: nothing."""
    maps, _ = _stacked_views(2)
    windows = [(0, 0, 9, 9, 0), (2, 5, 7, 6, 1)]
    med, mean = _merge(maps, windows, EDGE, "median").cpu(), _merge(maps, windows, EDGE, "mean").cpu()
    assert torch.equal(med, mean)
    r64 = merge_restatement(maps, windows, EDGE, "median", True, torch.float64)
    assert float((med.double() - r64).abs().max()) <= 1e-5
    assert bool((med[:, :, 11:] == 0.5).all()) and bool((med[:, :2, 9:] == 0.5).all())
    assert not bool((med[:, :, :9] == 0.5).all(0).any())
    u8 = _merge(maps, windows, EDGE, "median", output="u8").cpu()
    assert bool((u8[:, 11:] == 127).all())
    assert torch.equal(u8, med.mul(255).to(torch.uint8).permute(1, 2, 0))


def test_two_images_in_one_call_equal_the_two_calls_and_two_runs_are_identical():
    maps, windows = _oasis_case()
    smaps, swins = _stacked_views(9)
    flat, views = _pack([smaps, maps], [swins, windows])
    for merger in ("median", "mean"):
        for output in ("f32", "u8"):
            both = pp.merge_normal_views_gpu(flat, views, [EDGE, SIZE], merger, True, output)
            again = pp.merge_normal_views_gpu(flat, views, [EDGE, SIZE], merger, True, output)
            assert torch.equal(both[0], again[0]) and torch.equal(both[1], again[1])
            assert torch.equal(both[0].cpu(), _merge(smaps, swins, EDGE, merger, True, output).cpu())
            assert torch.equal(both[1].cpu(), _oasis_got(merger, True, output))


def test_non_finite_inputs_leave_the_pixels_they_do_not_reach_alone():
    maps, windows = _stacked_views(9)
    bad = [m.clone() for m in maps]
    for k, v in enumerate((float("nan"), float("inf"), -float("inf"))):
        bad[k][:, :, :8] = v                                                              # the left third of three maps
    for merger in ("median", "mean"):
        got = _merge(bad, windows, EDGE, merger).cpu()                                    # completes: nothing to index by a value
        clean = _merge(maps, windows, EDGE, merger).cpu()
        # plain views read columns <= 8 for output columns <= 4, flipped ones for columns >= 8
        assert torch.equal(got[:, :, 6:7], clean[:, :, 6:7])
        assert _merge(bad, windows, EDGE, merger, output="u8").shape == (*EDGE, 3)


# ------------------------------------------------------------------------------------------------ end to end
PRESET = [(1.0, [64], True), (0.8, [64], True)]


@functools.lru_cache(maxsize=None)
def _model():
    from omnidata_amd.model import build_model
    return build_model("normal", random_weights=0, dtype="bf16", max_batch=8).to(DEV)


def _rgb(h, w, seed):
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


def test_normals_tta_is_the_pieces_called_by_hand():
    from omnidata_amd.tta import NormalsTTA
    model, img = _model(), _rgb(96, 128, 1)
    plan = plan_views(128, 96, PRESET)
    assert len(plan) == 12 and {net for _, _, _, net in plan} == {(64, 96)}
    for merger, output in (("median", "u8"), ("mean", "f32")):
        got = NormalsTTA(model, PRESET, merger, batch_size=8)([img], output=output)
        assert len(got) == 1 and got[0].is_cuda and got[0].shape == ((96, 128, 3) if output == "u8" else (3, 96, 128))
        buf, descs = pp.pack_images([img])
        x = pp.views_to_input_gpu(buf.to(DEV), [pp.window_desc(descs[0], box) for box, _, _, _ in plan], [f for _, f, _, _ in plan],
                                  (64, 96))
        with torch.no_grad():
            y = torch.cat([model(x[:8]), model(x[8:])]).contiguous()                      # the model's own outputs
        views = [pp.TtaView(4 * k * 3 * 64 * 96, 64, 96, 0, *win) for k, win in enumerate(_windows_of(plan))]
        want = pp.merge_normal_views_gpu(y, views, [(96, 128)], merger, True, output)[0]
        assert torch.equal(got[0], want), (merger, output)
    assert not torch.equal(NormalsTTA(model, PRESET)([img])[0], NormalsTTA(model, PRESET, "mean")([img])[0])


def test_batch_predictor_routes_through_tta_in_input_order(tmp_path):
    from omnidata_amd.batch_infer import BatchPredictor
    from omnidata_amd.tta import NormalsTTA
    model = _model()
    shapes = [("a", (96, 128)), ("b", (120, 70))]
    (tmp_path / "in").mkdir()
    files = []
    for k, (stem, (h, w)) in enumerate(shapes):
        files.append(str(tmp_path / "in" / f"{stem}.png"))
        _rgb(h, w, 10 + k).save(files[-1])
    bp = BatchPredictor(model, "normal", batch_size=8, tta=PRESET)
    outs = list(bp.predict(files))
    alone = NormalsTTA(model, PRESET, batch_size=8)
    for f, (stem, (h, w)), o in zip(files, shapes, outs):
        assert o.shape == (h, w, 3) and o.dtype == torch.uint8
        assert torch.equal(o, alone([Image.open(f)])[0]), stem
    bp.predict_to_dir(files[::-1], str(tmp_path / "out"))
    for f, (stem, (h, w)), o in zip(files, shapes, outs):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / f"{stem}_normal.png")), o.cpu().numpy()), stem
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / f"{stem}_rgb.png")), np.asarray(Image.open(f))), stem
    with pytest.raises(ValueError):
        BatchPredictor(model, "depth", tta="flip")
    with pytest.raises(ValueError):
        BatchPredictor(model, "normal", tta="flip", full_frame="aspect")


def test_demo_cli_tta_flip_writes_files_of_the_images_own_sizes(tmp_path):
    shapes = [("a", (400, 520)), ("b", (390, 300))]
    (tmp_path / "in").mkdir()
    for k, (stem, (h, w)) in enumerate(shapes):
        _rgb(h, w, 20 + k).save(tmp_path / "in" / f"{stem}.png")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo.py"), "--task", "normal", "--img_path", str(tmp_path / "in"),
                        "--output_path", str(out), "--random-weights", "0", "--dtype", "bf16", "--tta", "flip"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for stem, (h, w) in shapes:
        assert Image.open(out / f"{stem}_normal.png").size == (w, h) and Image.open(out / f"{stem}_rgb.png").size == (w, h)
