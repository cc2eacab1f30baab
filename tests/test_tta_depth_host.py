"""Host side of test-time augmentation for depth (omnidata_amd/tta.py DepthTTA, csrc/tta_depth.hip): the conditions the shared
40-view fixture keeps, what the alignment buys on it, the anchor of a plan, the header against the library, the argument checks
of the three entry points (they return before anything touches a GPU), and the argument rules of BatchPredictor and demo.py."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from omnidata_amd import preprocess as pp
from omnidata_amd import tta
from tta_depth_restatement import (SIZE, align_merge_restatement, image_truth, oasis_depth_case, oasis_depth_reference,
                                   planted_coeffs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
PTR = 0x10000   # a non-null "device pointer": an argument check must reject the call before it is ever used
NORMAL_U8, NORMAL_F32, DEPTH_F32, DEPTH_RGBA, RENORM = 1, 2, 3, 4, 16


@pytest.fixture(scope="module")
def lib(built_lib):
    from omnidata_amd.engine import load_library
    return load_library()


# ------------------------------------------------------------------------------------------------ the fixture and the restatement
def test_the_forty_view_fixture_keeps_its_conditions():
    maps, windows, anchor = oasis_depth_case()
    assert len(maps) == 40 and windows[anchor] == (0, 0, *SIZE, 0)
    assert all(0.0 < float(m.min()) and float(m.max()) < 1.0 for m in maps)              # no clamped value
    for merger in ("median", "mean"):
        assert oasis_depth_reference(merger)[4] >= 0.01                                   # det / (n sum r^2) of every view


def test_fp64_restatement_recovers_the_planted_coefficients_and_the_anchor_is_the_identity():
    _, _, anchor = oasis_depth_case()
    c64 = oasis_depth_reference("median")[1]
    planted = torch.tensor([planted_coeffs(k, k == anchor) for k in range(40)], dtype=torch.float64)
    ds, db = float((c64[:, 0] - planted[:, 0]).abs().max()), float((c64[:, 1] - planted[:, 1]).abs().max())
    print(f"planted coefficients recovered to {ds:.2e} (scale) {db:.2e} (shift)")
    assert ds <= 0.02 and db <= 0.01
    assert c64[anchor].tolist() == [1.0, 0.0]


@pytest.mark.parametrize("merger", ["median", "mean"])
def test_aligned_merge_is_at_least_four_times_closer_to_the_truth_than_the_unaligned_one(merger):
    truth = image_truth(SIZE)
    aligned = float(((1 - oasis_depth_reference(merger)[0]) - truth).abs().mean())
    unaligned = float(((1 - oasis_depth_reference(merger, align=False)[0]) - truth).abs().mean())
    print(f"{merger}: mean |merged - truth| {aligned:.2e} aligned, {unaligned:.2e} unaligned")
    assert aligned <= unaligned / 4


def test_degenerate_views_one_pixel_windows_and_uncovered_pixels_in_the_restatement():
    a = torch.linspace(0.2, 0.8, 6 * 8, dtype=torch.float32).reshape(6, 8)
    flat = torch.full((4, 4), 0.3)
    out, coeffs = align_merge_restatement([a, flat, flat[:1, :1] * 2], [(0, 0, 6, 8, 0), (1, 2, 4, 4, 0), (5, 7, 1, 1, 0)], (6, 8), 0,
                                          "mean", torch.float64)
    assert coeffs[0].tolist() == [1.0, 0.0] and float(coeffs[1, 0]) == 1.0 and float(coeffs[2, 0]) == 1.0
    assert abs(float(coeffs[1, 1]) - (float(a[1:5, 2:6].double().mean()) - float(flat[0, 0]))) <= 1e-12
    assert abs(float(out[5, 7]) - (1 - float(a[5, 7]))) <= 1e-12                         # the 1 x 1 view lands on the anchor
    out, _ = align_merge_restatement([flat], [(1, 2, 4, 4, 0)], (6, 8), 0, "median", torch.float64, align=False)
    assert float(out[0, 0]) == 1.0 and abs(float(out[2, 3]) - (1 - float(flat[0, 0]))) <= 1e-12   # nothing covers (0, 0): 1 - 0


# ------------------------------------------------------------------------------------------------ plan
def test_anchor_selection_and_the_prepended_anchor(monkeypatch):
    for preset, n in (("flip", 2), ("whole", 10)):
        plan, anchor = tta.plan_depth_views(640, 480, preset)
        assert plan == tta.plan_views(640, 480, preset) and len(plan) == n and anchor == 0
    plan, anchor = tta.plan_depth_views(683, 512, "oasis")
    assert len(plan) == 40 and anchor == 30 and plan[30][:2] == ((0, 0, 683, 512), False)
    plan, anchor = tta.plan_depth_views(640, 480, "crops")
    assert len(plan) == 21 and anchor == 0 and plan[1:] == tta.plan_views(640, 480, "crops")
    assert plan[0] == ((0, 0, 640, 480), False, 384, (384, 512))
    assert tta.plan_depth_views(2000, 300, "crops")[0][0][3] == (384, 1024)               # the anchor's network size is cut back too
    assert tta.plan_depth_views(640, 480, "crops", multiple=64, max_side=512)[0][0][3] == (384, 512)
    plan, anchor = tta.plan_depth_views(96, 128, [(1.0, [64], False), (0.8, [64], True)])
    assert anchor == 0 and len(plan) == 11
    # a flipped whole-image view is no anchor; 64 views without one leave no room for it
    mirrored = [((0, 0, 640, 480), True, 64, (64, 96))]
    monkeypatch.setattr(tta, "plan_views", lambda *a, **k: mirrored * 63)
    plan, anchor = tta.plan_depth_views(640, 480, "whole")
    assert len(plan) == 64 and anchor == 0 and plan[0][1] is False
    monkeypatch.setattr(tta, "plan_views", lambda *a, **k: mirrored * 64)
    with pytest.raises(ValueError):
        tta.plan_depth_views(640, 480, "whole")


# ------------------------------------------------------------------------------------------------ header
def test_header_declares_the_three_entry_points_and_the_library_exports_them(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dptx.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", text)
    for proto in ("int dptx_tta_depth_workspace_bytes(const dptx_tta_view* views, int32_t n_views, const dptx_image_desc* outs, "
                  "int32_t B, int64_t* bytes);",
                  "int dptx_tta_align_depth(const void* views_dev, const dptx_tta_view* views, int32_t n_views, const int32_t* anchors, "
                  "const dptx_image_desc* outs, int32_t B, float* coeffs_dev, void* ws, int64_t ws_bytes, void* stream);",
                  "int dptx_tta_merge_depth(const void* views_dev, const dptx_tta_view* views, int32_t n_views, const float* coeffs_dev, "
                  "const dptx_image_desc* outs, int32_t B, int32_t mode, void* out_dev, const void* ws, void* stream);"):
        assert proto in flat, proto
    defines = {n: int(v) for n, v in re.findall(r"^#define (DPTX_\w+) (\d+)\s*$", text, flags=re.M)}
    assert defines["DPTX_RESIZE_DEPTH_F32"] == pp.RESIZE_MODES["depth_f32"] == DEPTH_F32
    assert defines["DPTX_TTA_MEAN"] == pp.TTA_MEAN and defines["DPTX_TTA_MAX_VIEWS"] == pp.TTA_MAX_VIEWS == 64
    for name in ("dptx_tta_depth_workspace_bytes", "dptx_tta_align_depth", "dptx_tta_merge_depth"):
        assert hasattr(lib, name)
    from omnidata_amd.build import HEADERS, SOURCES
    assert "tta_depth.hip" in SOURCES and "tta_common.h" in HEADERS
    assert "out of scope" not in tta.__doc__ and "compute_scale_and_shift" in tta.__doc__


# ------------------------------------------------------------------------------------------------ argument checks
def _view(image=0, offset=0, h=64, w=96, y0=0, x0=0, ch=70, cw=93, flip=0):
    return pp.TtaView(offset, h, w, image, y0, x0, ch, cw, flip)


def _out(H=70, W=93, stride=None, offset=0):
    return pp.ImageDesc(offset, H, W, 1, W * 4 if stride is None else stride)


def _calls(lib, views, outs, anchors=(0,), mode=DEPTH_F32, n_views=None, B=None, maps=PTR, out=PTR, coeffs=PTR, ws=PTR, ws_bytes=1 << 40,
           views_null=False, outs_null=False, anchors_null=False):
    """-> the return codes of (workspace_bytes, align, merge) for one set of arguments"""
    va = (pp.TtaView * max(len(views), 1))(*views)
    oa = (pp.ImageDesc * max(len(outs), 1))(*outs)
    an = (C.c_int32 * max(len(anchors), 1))(*anchors)
    vp, op = None if views_null else C.addressof(va), None if outs_null else C.addressof(oa)
    nv, nb = len(views) if n_views is None else n_views, len(outs) if B is None else B
    nbytes = C.c_int64(-1)
    return (lib.dptx_tta_depth_workspace_bytes(vp, nv, op, nb, C.byref(nbytes)),
            lib.dptx_tta_align_depth(maps, vp, nv, None if anchors_null else C.addressof(an), op, nb, coeffs, ws, ws_bytes, None),
            lib.dptx_tta_merge_depth(maps, vp, nv, coeffs, op, nb, mode, out, ws, None))


def test_the_three_entry_points_reject_bad_arguments_without_a_gpu(lib):
    good, whole = _out(), _view()
    every = (INVALID, INVALID, INVALID)
    # what dptx_tta_merge_normals rejects of the views and the outputs, in all three
    assert _calls(lib, [whole] * 65, [good]) == every                                      # 65 views for one image
    assert _calls(lib, [_view(y0=1)], [good]) == every                                     # a window outside the image
    assert _calls(lib, [_view(x0=1)], [good]) == every
    assert _calls(lib, [_view(y0=-1, ch=10)], [good]) == every
    assert _calls(lib, [_view(ch=0)], [good]) == every
    assert _calls(lib, [_view(cw=94)], [good]) == every
    assert _calls(lib, [whole, _view(image=1), whole], [good, good], anchors=(0, 1)) == every     # views not grouped by image
    assert _calls(lib, [_view(image=1), whole], [good, good], anchors=(1, 0)) == every     # images not ascending
    assert _calls(lib, [whole, _view(image=2)], [good, good, good], anchors=(0, 0, 1)) == every   # an image without a view
    assert _calls(lib, [_view(image=-1)], [good]) == every
    assert _calls(lib, [_view(offset=2)], [good]) == every                                 # a misaligned offset
    assert _calls(lib, [_view(offset=-4)], [good]) == every
    assert _calls(lib, [_view(h=0)], [good]) == every
    assert _calls(lib, [_view(w=4097)], [good]) == every
    assert _calls(lib, [_view(ch=16385)], [_out(H=16385)]) == every
    assert _calls(lib, [whole], [_out(stride=93 * 4 + 2)]) == every                        # fp32 rows: stride and offset in dwords
    assert _calls(lib, [whole], [_out(offset=2)]) == every
    assert _calls(lib, [whole], [_out(stride=93 * 4 - 4)]) == every
    assert _calls(lib, [whole], [good], B=0) == every
    assert _calls(lib, [whole], [good], n_views=0) == every
    assert _calls(lib, [whole], [good], B=4097) == every
    assert _calls(lib, [whole], [good], views_null=True) == every
    assert _calls(lib, [whole], [good], outs_null=True) == every
    # device pointers: the two entries that take them
    assert _calls(lib, [whole], [good], maps=None)[1:] == (INVALID, INVALID)
    assert _calls(lib, [whole], [good], maps=PTR + 2)[1:] == (INVALID, INVALID)
    assert _calls(lib, [whole], [good], coeffs=PTR + 2)[1:] == (INVALID, INVALID)
    assert _calls(lib, [whole], [good], out=None)[2] == INVALID
    assert _calls(lib, [whole], [good], out=PTR + 1)[2] == INVALID
    assert _calls(lib, [whole], [good], coeffs=None)[1] == INVALID                         # align has to write them
    assert _calls(lib, [whole], [good], ws=None)[1] == INVALID
    assert _calls(lib, [whole], [good], ws=PTR + 4)[1] == INVALID
    assert _calls(lib, [whole], [good], anchors_null=True)[1] == INVALID
    # the anchor: a view of its image that covers the whole of it
    crop = _view(y0=3, x0=5, ch=60, cw=80)
    assert _calls(lib, [whole, crop], [good], anchors=(1,))[1] == INVALID                  # does not cover the image
    assert _calls(lib, [_view(ch=69), crop], [good], anchors=(0,))[1] == INVALID
    assert _calls(lib, [_view(cw=92), crop], [good], anchors=(0,))[1] == INVALID
    assert _calls(lib, [whole, crop], [good], anchors=(2,))[1] == INVALID                  # not a view at all
    assert _calls(lib, [whole, crop], [good], anchors=(-1,))[1] == INVALID
    assert _calls(lib, [whole, _view(image=1)], [good, good], anchors=(0, 0))[1] == INVALID   # a view of another image
    assert _calls(lib, [whole, _view(image=1)], [good, good], anchors=(1, 0))[1] == INVALID
    # the workspace: exactly what the host-only entry asks for
    va, oa, nbytes = (pp.TtaView * 2)(whole, crop), (pp.ImageDesc * 1)(good), C.c_int64()
    assert lib.dptx_tta_depth_workspace_bytes(C.addressof(va), 2, C.addressof(oa), 1, C.byref(nbytes)) == 0
    plane = (70 * 93 * 4 + 255) // 256 * 256
    records = (2 * 5 + 2 * 4) * 32                                                         # 64 x 16 tiles of 70 x 93 and of 60 x 80
    assert nbytes.value == plane + (records + 255) // 256 * 256
    assert lib.dptx_tta_depth_workspace_bytes(C.addressof(va), 2, C.addressof(oa), 1, None) == INVALID
    assert _calls(lib, [whole, crop], [good], ws_bytes=nbytes.value - 1)[1] == INVALID
    # the mode: DPTX_RESIZE_DEPTH_F32, | DPTX_TTA_MEAN, nothing else
    for mode in (0, NORMAL_U8, NORMAL_F32, DEPTH_RGBA, DEPTH_F32 | RENORM, DEPTH_F32 | pp.TTA_RAW_VIEWS, DEPTH_F32 | 128, pp.TTA_MEAN, -1):
        assert _calls(lib, [whole], [good], mode=mode)[2] == INVALID


# ------------------------------------------------------------------------------------------------ argument rules above the library
class _NoModel:
    """Stands where a model goes: every rule below must be decided before the model is touched."""

    def parameters(self):
        raise AssertionError("the model was touched before the arguments were checked")


def test_batch_predictor_argument_rules():
    from omnidata_amd.batch_infer import BatchPredictor
    model = _NoModel()
    with pytest.raises(ValueError, match="tta_align"):
        BatchPredictor(model, "depth", tta="flip")                                        # depth needs the alignment step
    with pytest.raises(ValueError, match="tta_align"):
        BatchPredictor(model, "normal", tta="flip", tta_align="lstsq")                    # normals have nothing to align
    with pytest.raises(ValueError, match="tta_align"):
        BatchPredictor(model, "depth", tta_align="lstsq")                                 # no tta
    with pytest.raises(ValueError, match="tta_align"):
        BatchPredictor(model, "depth", tta="flip", tta_align="affine")
    with pytest.raises(ValueError):
        BatchPredictor(model, "depth", tta="flip", tta_align="lstsq", full_frame="aspect")
    with pytest.raises(ValueError):
        BatchPredictor(model, "normal", tta="flip", full_frame="aspect")
    with pytest.raises(ValueError, match="DPT depth model"):
        tta.DepthTTA(model)                                                               # DPT depth models only (no UNet, no normals)
    for kw in (dict(merger="mode"), dict(align="affine"), dict(batch_size=0), dict(chunk_images=0)):
        with pytest.raises(ValueError):
            tta.DepthTTA(model, **kw)


@pytest.mark.parametrize("argv,message", [
    (["--task", "depth", "--tta", "whole"], "--tta_align lstsq"),
    (["--task", "normal", "--tta", "whole", "--tta_align", "lstsq"], "--tta_align needs --task depth"),
    (["--task", "depth", "--tta_align", "lstsq"], "--tta_align needs --task depth and --tta"),
    (["--task", "depth", "--tta", "whole", "--tta_align", "lstsq", "--backbone", "unet"], "--backbone unet --task depth has no --tta"),
    (["--task", "depth", "--tta", "whole", "--tta_align", "lstsq", "--full_frame", "aspect"], "--tta excludes --full_frame"),
])
def test_demo_cli_refuses_before_it_builds_a_model(argv, message, tmp_path, capsys, monkeypatch):
    monkeypatch.syspath_prepend(ROOT)
    import demo
    with pytest.raises(SystemExit):
        demo.main(argv + ["--img_path", str(tmp_path), "--output_path", str(tmp_path / "out")])
    assert message in capsys.readouterr().out
    assert not (tmp_path / "out").exists()
    with pytest.raises(SystemExit):
        demo.main(["--task", "depth", "--tta", "whole", "--tta_align", "affine", "--img_path", str(tmp_path), "--output_path", str(tmp_path)])
