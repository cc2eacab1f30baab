"""Test-time augmentation for depth on the GPU (csrc/tta_depth.hip, omnidata_amd/tta.py DepthTTA): the alignment and the merge
against their restatement (tests/tta_depth_restatement.py), the edges of the selection and of the fit, determinism, and the
pipeline end to end.  pytest -m gpu.

Measured on an MI355X: profiles/tta_depth_parity.md."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from omnidata_amd import preprocess as pp
from omnidata_amd.tta import plan_depth_views
from tta_depth_restatement import (EDGE, SIZE, oasis_depth_case, oasis_depth_reference, stacked_depth_case,
                                   stacked_depth_reference, windows_of)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH_F32 = 3
BOUND_ABS = 2e-6            # the project's bound for a bilinear resize (tests/test_gpu_fullframe.py)


def _lib():
    from omnidata_amd.engine import load_library
    return load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pack(maps_per_image, windows_per_image, anchors_per_image):
    """-> (flat fp32 device tensor, [TtaView], anchors as indices into the views): every map back to back, image-major."""
    views, chunks, off, anchors = [], [], 0, []
    for i, (maps, windows, anchor) in enumerate(zip(maps_per_image, windows_per_image, anchors_per_image)):
        anchors.append(len(views) + anchor)
        for m, (y0, x0, ch, cw, flip) in zip(maps, windows):
            views.append(pp.TtaView(4 * off, m.shape[0], m.shape[1], i, y0, x0, ch, cw, flip))
            chunks.append(m.reshape(-1))
            off += m.numel()
    return torch.cat(chunks).to(DEV), views, anchors


def _align_merge(maps, windows, anchor, size, merger="median", align=True):
    """-> (out [H,W] on the host, coeffs [views, 2] on the host or None)"""
    flat, views, anchors = _pack([maps], [windows], [anchor])
    coeffs = ws = None
    if align:
        coeffs, ws = pp.align_depth_views_gpu(flat, views, anchors, [size])
    out = pp.merge_depth_views_gpu(flat, views, [size], coeffs, ws, merger, "f32")[0]
    return out.cpu(), None if coeffs is None else coeffs.cpu()


@functools.lru_cache(maxsize=None)
def _oasis_got(merger):
    maps, windows, anchor = oasis_depth_case()
    return _align_merge(maps, windows, anchor, SIZE, merger)


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("merger", ["median", "mean"])
def test_forty_views_coefficients_and_merge_within_twice_the_restatements_own_rounding(merger):
    """e_ref / e_ref_c = max|fp32 restatement - fp64 restatement| of the output / the coefficients; required:
    max|got - fp64 restatement| <= 2 * e_ref + 2e-6 for both (a wrong tap, a missing view or a wrong sum is >= 1e-3).  Views of
    70 x 93 and 63 x 84 windows span 10 and 8 blocks of the stats pass: the records and the solve's strided sum are in it."""
    r64, c64, e_ref, e_ref_c, flattest = oasis_depth_reference(merger)
    out, coeffs = _oasis_got(merger)
    err, err_c = float((out.double() - r64).abs().max()), float((coeffs.double() - c64).abs().max())
    print(f"tta depth parity {merger} {SIZE} 40 views: e_ref {e_ref:.3e} err {err:.3e} err / (2 e_ref + 2e-6) = "
          f"{err / (2 * e_ref + BOUND_ABS):.3f}; e_ref_c {e_ref_c:.3e} err_c {err_c:.3e} err_c / (2 e_ref_c + 2e-6) = "
          f"{err_c / (2 * e_ref_c + BOUND_ABS):.3f}; flattest view det / (n sum r^2) {flattest:.4f}")
    assert out.shape == r64.shape == SIZE and coeffs.shape == (40, 2)
    assert err_c <= 2 * e_ref_c + BOUND_ABS, (merger, err_c, e_ref_c)
    assert err <= 2 * e_ref + BOUND_ABS, (merger, err, e_ref)


@pytest.mark.parametrize("n", [1, 2, 3, 8, 9, 16, 17, 32, 33, 63, 64])
def test_every_count_up_to_64_on_one_pixel_class(n):
    """One view, both sides of every views-per-image class (8 / 16 / 32 / 64), odd and even counts; median and mean."""
    maps, windows, anchor = stacked_depth_case(n)
    for merger in ("median", "mean"):
        r64, c64, e_ref, e_ref_c = stacked_depth_reference(n, merger)
        out, coeffs = _align_merge(maps, windows, anchor, EDGE, merger)
        err, err_c = float((out.double() - r64).abs().max()), float((coeffs.double() - c64).abs().max())
        print(f"tta depth parity {merger} {n} stacked views: e_ref {e_ref:.3e} err {err:.3e}; e_ref_c {e_ref_c:.3e} err_c {err_c:.3e}")
        assert err_c <= 2 * e_ref_c + BOUND_ABS, (n, merger, err_c, e_ref_c)
        assert err <= 2 * e_ref + BOUND_ABS, (n, merger, err, e_ref)


# ------------------------------------------------------------------------------------------------ edges of the fit
def test_anchor_is_exactly_the_identity_a_constant_view_gets_scale_one_and_a_one_pixel_window_lands_on_the_anchor():
    maps, windows, _ = stacked_depth_case(2)
    anchor_map = maps[0]
    flat_map = torch.full((16, 24), 0.3)
    one = torch.full((1, 1), 0.9)
    wins = [(0, 0, *EDGE, 0), (2, 3, 5, 7, 1), (4, 6, 1, 1, 0)]
    out, coeffs = _align_merge([anchor_map, flat_map, one], wins, 0, EDGE, "median")
    assert _oasis_got("median")[1][30].tolist() == [1.0, 0.0] and coeffs[0].tolist() == [1.0, 0.0]
    a = F.interpolate(anchor_map[None, None].double(), EDGE, mode="bilinear", align_corners=False)[0, 0]
    assert float(coeffs[1, 0]) == 1.0                                                     # flatter than 1e-5 of its own level
    assert abs(float(coeffs[1, 1]) - (float(a[2:7, 3:10].mean()) - 0.3)) <= BOUND_ABS     # the mean difference
    assert float(coeffs[2, 0]) == 1.0 and abs(float(coeffs[2, 1]) - (float(a[4, 6]) - 0.9)) <= BOUND_ABS
    # (4, 6): anchor, constant view and the 1 x 1 view; the last is the anchor's value there, so the median is too
    assert abs(float(out[4, 6]) - (1 - float(a[4, 6]))) <= BOUND_ABS
    only, c = _align_merge([anchor_map, one], [wins[0], wins[2]], 0, EDGE, "mean")
    assert abs(float(only[4, 6]) - (1 - float(a[4, 6]))) <= BOUND_ABS
    assert float((only.double() - (1 - a)).abs().max()) <= BOUND_ABS


def test_without_coefficients_the_merge_is_the_unaligned_restatement_and_one_view_is_interpolate():
    maps, windows, anchor = oasis_depth_case()
    for merger in ("median", "mean"):
        r64, _, e_ref, _, _ = oasis_depth_reference(merger, align=False)
        out, coeffs = _align_merge(maps, windows, anchor, SIZE, merger, align=False)
        assert coeffs is None
        assert float((out.double() - r64).abs().max()) <= 2 * e_ref + BOUND_ABS, merger
        assert float((out - _oasis_got(merger)[0]).abs().max()) >= 1e-3                   # the alignment is not a no-op here
    m = maps[anchor] * 3 - 1                                                              # leaves [0, 1] on both sides
    assert float(m.min()) < 0 and float(m.max()) > 1
    want = 1 - F.interpolate(m[None, None].double().clamp(0, 1), SIZE, mode="bilinear", align_corners=False)[0, 0]
    for merger in ("median", "mean"):
        out, _ = _align_merge([m], [(0, 0, *SIZE, 0)], 0, SIZE, merger, align=False)
        assert float((out.double() - want).abs().max()) <= BOUND_ABS
    # no anchor and no view at a pixel: 0 before the inversion
    out, _ = _align_merge([maps[anchor]], [(3, 5, 20, 30, 0)], 0, SIZE, "median", align=False)
    assert bool((out[:3] == 1).all()) and bool((out[:, :5] == 1).all()) and bool((out[3:23, 5:35] < 1).all())


# ------------------------------------------------------------------------------------------------ determinism
def test_two_images_in_one_call_equal_the_two_calls_and_two_runs_are_identical():
    big, big_w, big_a = oasis_depth_case()
    small, small_w, small_a = stacked_depth_case(9)
    flat, views, anchors = _pack([small, big], [small_w, big_w], [small_a, big_a])
    coeffs, ws = pp.align_depth_views_gpu(flat, views, anchors, [EDGE, SIZE])
    again, _ = pp.align_depth_views_gpu(flat, views, anchors, [EDGE, SIZE])
    assert torch.equal(coeffs, again)
    for merger in ("median", "mean"):
        both = pp.merge_depth_views_gpu(flat, views, [EDGE, SIZE], coeffs, ws, merger)
        twice = pp.merge_depth_views_gpu(flat, views, [EDGE, SIZE], again, None, merger)
        assert torch.equal(both[0], twice[0]) and torch.equal(both[1], twice[1])
        alone_small = _align_merge(small, small_w, small_a, EDGE, merger)
        assert torch.equal(both[0].cpu(), alone_small[0]) and torch.equal(coeffs[:9].cpu(), alone_small[1])
        assert torch.equal(both[1].cpu(), _oasis_got(merger)[0]) and torch.equal(coeffs[9:].cpu(), _oasis_got(merger)[1])


def test_the_views_per_image_class_does_not_change_a_bit():
    """min / max move values and never round them: the same 5 covering views inside sets of 5, 9, 17 and 33 views (the kernel's
    four classes) whose extra views lie in a 14th column give the same bits in the first 13, coefficients included."""
    maps, windows, _ = stacked_depth_case(33)
    size = (EDGE[0], EDGE[1] + 1)                                                          # a 14th column for the extra views
    anchor_map = maps[0]
    want = None
    for n in (5, 9, 17, 33):
        wins = [(0, 0, *size, 0)] + list(windows[1:5]) + [(0, EDGE[1], EDGE[0], 1, 0)] * (n - 5)
        out, coeffs = _align_merge([anchor_map] + list(maps[1:n]), wins, 0, size, "median")
        got = (out[:, :EDGE[1]], coeffs[:5])
        want = got if want is None else want
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), n


def test_canaries_around_a_strided_output_stay():
    big, big_w, big_a = oasis_depth_case()
    small, small_w, small_a = stacked_depth_case(9)
    flat, views, anchors = _pack([big, small], [big_w, small_w], [big_a, small_a])
    sizes = [SIZE, EDGE]
    coeffs, ws = pp.align_depth_views_gpu(flat, views, anchors, sizes)
    tight = pp.merge_depth_views_gpu(flat, views, sizes, coeffs, ws, "median")
    descs, off, spans = (pp.ImageDesc * 2)(), 4, []
    for i, (H, W) in enumerate(sizes):
        stride = W * 4 + 4 * (1 + i)
        descs[i] = pp.ImageDesc(off, H, W, 1, stride)
        spans.append((off, H, W * 4, stride))
        off += H * stride + 8
    buf = torch.full((off + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    arr = (pp.TtaView * len(views))(*views)
    assert _lib().dptx_tta_merge_depth(flat.data_ptr(), C.addressof(arr), len(views), coeffs.data_ptr(), C.addressof(descs), 2, DEPTH_F32,
                                       buf.data_ptr(), ws.data_ptr(), _stream()) == 0
    host = buf.cpu().numpy()
    owned = np.zeros(host.shape, dtype=bool)
    for (o, rows, rowbytes, stride), t, (H, W) in zip(spans, tight, sizes):
        idx = o + np.arange(rows)[:, None] * stride + np.arange(rowbytes)[None, :]
        owned[idx] = True
        assert np.array_equal(np.ascontiguousarray(host[idx]).view(np.float32).reshape(H, W), t.cpu().numpy())   # padded == tight
    assert (host[~owned] == 0xA5).all()
    # the alignment writes the coefficients of its views and nothing next to them
    guarded = torch.full((len(views) + 2, 2), 7.0, device=DEV)
    anc = (C.c_int32 * 2)(*anchors)
    tight_descs, _ = pp.output_layout(sizes, "depth_f32")
    assert _lib().dptx_tta_align_depth(flat.data_ptr(), C.addressof(arr), len(views), C.addressof(anc), C.addressof(tight_descs), 2,
                                       guarded[1:].data_ptr(), ws.data_ptr(), ws.numel(), _stream()) == 0
    assert torch.equal(guarded[1:-1], coeffs) and bool((guarded[0] == 7).all()) and bool((guarded[-1] == 7).all())


def test_non_finite_values_in_one_images_views_leave_the_other_image_alone():
    big, big_w, big_a = oasis_depth_case()
    small, small_w, small_a = stacked_depth_case(9)
    bad = [m.clone() for m in small]
    for k, v in enumerate((float("nan"), float("inf"), -float("inf"))):
        bad[k + 1][:, :8] = v
    bad[0][3, 3] = float("nan")                                                           # the anchor too
    flat, views, anchors = _pack([bad, big], [small_w, big_w], [small_a, big_a])
    coeffs, ws = pp.align_depth_views_gpu(flat, views, anchors, [EDGE, SIZE])             # completes: nothing is indexed by a value
    for merger in ("median", "mean"):
        both = pp.merge_depth_views_gpu(flat, views, [EDGE, SIZE], coeffs, ws, merger)
        assert both[0].shape == EDGE
        assert torch.equal(both[1].cpu(), _oasis_got(merger)[0])
    assert torch.equal(coeffs[9:].cpu(), _oasis_got("median")[1])
    assert pp.merge_depth_views_gpu(flat, views, [EDGE, SIZE], coeffs, ws, "median", "rgba")[0].shape == (*EDGE, 4)


# ------------------------------------------------------------------------------------------------ end to end
PRESET = [(1.0, [64], True), (0.8, [64], True)]


@functools.lru_cache(maxsize=None)
def _model():
    from omnidata_amd.model import build_model
    return build_model("depth", random_weights=0, dtype="bf16", max_batch=8).to(DEV)


def _rgb(h, w, seed):
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


def test_depth_tta_is_the_pieces_called_by_hand():
    from omnidata_amd.tta import DepthTTA
    model, img = _model(), _rgb(96, 128, 1)
    plan, anchor = plan_depth_views(128, 96, PRESET)
    assert len(plan) == 12 and anchor == 0 and {net for _, _, _, net in plan} == {(64, 96)}
    buf, descs = pp.pack_images([img])
    x = pp.views_to_input_gpu(buf.to(DEV), [pp.window_desc(descs[0], box) for box, _, _, _ in plan], [f for _, f, _, _ in plan],
                              (64, 96), "depth")
    with torch.no_grad():
        y = torch.cat([model(x[:8]), model(x[8:])]).contiguous()                          # the model's own outputs, [12,64,96]
    assert y.shape == (12, 64, 96)
    views = [pp.TtaView(4 * k * 64 * 96, 64, 96, 0, *win) for k, win in enumerate(windows_of(plan))]
    coeffs, ws = pp.align_depth_views_gpu(y, views, [anchor], [(96, 128)])
    for merger, output in (("median", "rgba"), ("mean", "f32"), ("median", "f32")):
        got, got_c = DepthTTA(model, PRESET, merger, batch_size=8)([img], output=output, return_coeffs=True)
        assert len(got) == 1 and got[0].is_cuda and got[0].shape == ((96, 128, 4) if output == "rgba" else (96, 128))
        want = pp.merge_depth_views_gpu(y, views, [(96, 128)], coeffs, ws, merger, output)[0]
        assert torch.equal(got[0], want), (merger, output)
        assert len(got_c) == 1 and torch.equal(got_c[0], coeffs)
    plain = DepthTTA(model, PRESET, align=None, batch_size=8)([img], output="f32")[0]
    assert torch.equal(plain, pp.merge_depth_views_gpu(y, views, [(96, 128)], None, None, "median", "f32")[0])


def test_batch_predictor_routes_depth_through_tta_in_input_order(tmp_path):
    from omnidata_amd.batch_infer import BatchPredictor
    from omnidata_amd.tta import DepthTTA
    model = _model()
    shapes = [("a", (96, 128)), ("b", (120, 70))]
    (tmp_path / "in").mkdir()
    files = []
    for k, (stem, (h, w)) in enumerate(shapes):
        files.append(str(tmp_path / "in" / f"{stem}.png"))
        _rgb(h, w, 10 + k).save(files[-1])
    bp = BatchPredictor(model, "depth", batch_size=8, tta=PRESET, tta_align="lstsq")
    outs = list(bp.predict(files))
    alone = DepthTTA(model, PRESET, batch_size=8)
    for f, (stem, (h, w)), o in zip(files, shapes, outs):
        assert o.shape == (h, w, 4) and o.dtype == torch.uint8
        assert torch.equal(o, alone([Image.open(f)])[0]), stem
    bp.predict_to_dir(files[::-1], str(tmp_path / "out"))
    for f, (stem, (h, w)), o in zip(files, shapes, outs):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / f"{stem}_depth.png")), o.cpu().numpy()), stem
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / f"{stem}_rgb.png")), np.asarray(Image.open(f))), stem
    with pytest.raises(ValueError, match="tta_align"):
        BatchPredictor(model, "depth", tta=PRESET)


def test_demo_cli_depth_tta_flip_writes_files_of_the_images_own_sizes(tmp_path):
    shapes = [("a", (400, 520)), ("b", (390, 300))]
    (tmp_path / "in").mkdir()
    for k, (stem, (h, w)) in enumerate(shapes):
        _rgb(h, w, 20 + k).save(tmp_path / "in" / f"{stem}.png")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo.py"), "--task", "depth", "--img_path", str(tmp_path / "in"),
                        "--output_path", str(out), "--random-weights", "0", "--dtype", "bf16", "--tta", "flip", "--tta_align", "lstsq"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for stem, (h, w) in shapes:
        depth = Image.open(out / f"{stem}_depth.png")
        assert depth.size == (w, h) and depth.mode == "RGBA" and Image.open(out / f"{stem}_rgb.png").size == (w, h)
