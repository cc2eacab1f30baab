"""Host side of test-time augmentation (omnidata_amd/tta.py, csrc/tta.hip, csrc/fullframe.hip): the view plan, the invariances
of the merge's restatement, the header against the ctypes tables, and the argument checks of the two entry points (they return
before anything touches a GPU)."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from omnidata_amd import preprocess as pp
from omnidata_amd.tta import PRESETS, five_crops, plan_views
from tta_restatement import merge_restatement, synthetic_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
PTR = 0x10000   # a non-null "device pointer": an argument check must reject the call before it is ever used
NORMAL_U8, NORMAL_F32, DEPTH_F32, RENORM = 1, 2, 3, 16


@pytest.fixture(scope="module")
def lib(built_lib):
    from omnidata_amd.engine import load_library
    return load_library()


# ------------------------------------------------------------------------------------------------ plan
def test_five_crops_windows_and_their_order():
    assert five_crops(93, 70, 0.8) == [(0, 0, 74, 56), (19, 0, 93, 56), (0, 14, 74, 70), (19, 14, 93, 70), (9, 7, 83, 63)]
    assert five_crops(683, 512, 0.9)[4] == ((683 - 615) // 2, (512 - 461) // 2, (683 - 615) // 2 + 615, (512 - 461) // 2 + 461)
    assert five_crops(5, 5, 0.5) == [(0, 0, 2, 2), (3, 0, 5, 2), (0, 3, 2, 5), (3, 3, 5, 5), (1, 1, 3, 3)]     # round(2.5) = 2
    assert five_crops(1, 1, 0.1) == [(0, 0, 1, 1)] * 5                                                         # never empty
    assert five_crops(40, 30, 1.0) == [(0, 0, 40, 30)]
    with pytest.raises(ValueError):
        five_crops(40, 30, 1.5)


def test_oasis_preset_has_the_scripts_40_views_in_the_stated_order():
    w, h = 683, 512
    views = plan_views(w, h, "oasis")
    assert len(views) == 40
    want = []
    for fraction, sides in ((0.8, [512]), (0.9, [512, 256]), (1.0, [512, 256, 320, 384, 448])):     # oasis_eval_tta.py:487-534
        for box in five_crops(w, h, fraction):
            for s in sides:
                want += [(box, False, s), (box, True, s)]
    assert [v[:3] for v in views] == want
    assert views[0][0] == (0, 0, 546, 410) and views[30][0] == (0, 0, w, h)
    for box, flip, s, (nh, nw) in views:
        left, top, right, bottom = box
        assert 0 <= left < right <= w and 0 <= top < bottom <= h
        assert nh % 32 == 0 and nw % 32 == 0 and 64 <= nh <= 1024 and 64 <= nw <= 1024
        assert (nw, nh) == pp.full_frame_net_size(right - left, bottom - top, s, 32)[:2]
        assert min(nh, nw) == s
    assert views[30][3] == (512, 672) and views[32][3] == (256, 352)


def test_the_other_presets_explicit_lists_and_the_unet_sizes():
    assert [len(plan_views(640, 480, p)) for p in ("flip", "whole", "crops")] == [2, 10, 20]
    assert [v[1:] for v in plan_views(640, 480, "flip")] == [(False, 384, (384, 512)), (True, 384, (384, 512))]
    assert len(plan_views(96, 128, [(1.0, [64], True), (0.8, [64], True)])) == 12
    assert [v[1] for v in plan_views(96, 128, [(0.8, [64, 96], False)])] == [False] * 10
    for w, h in ((683, 512), (512, 683), (2000, 300), (300, 2000)):
        for box, flip, s, (nh, nw) in plan_views(w, h, "oasis", multiple=64, max_side=512):
            assert nh % 64 == 0 and nw % 64 == 0 and 64 <= nh <= 512 and 64 <= nw <= 512
        for box, flip, s, (nh, nw) in plan_views(w, h, "oasis"):
            assert nh % 32 == 0 and nw % 32 == 0 and nh <= 1024 and nw <= 1024
    assert plan_views(2000, 300, "flip")[0][3] == (384, 1024)                                   # 2560 wide -> cut back
    with pytest.raises(ValueError):
        plan_views(640, 480, "fivecrops")
    with pytest.raises(ValueError):
        plan_views(640, 480, [(0.8, [64, 96, 128, 160, 192, 224, 256], True)])                  # 70 views > 64
    assert set(PRESETS) == {"flip", "whole", "crops", "oasis"}


# ------------------------------------------------------------------------------------------------ the restatement
SIZE = (35, 47)


def _small_case():
    windows = [(0, 0, 35, 47, 0), (0, 0, 35, 47, 1), (3, 5, 28, 38, 0), (7, 9, 28, 38, 1), (0, 9, 20, 38, 0)]
    shapes = [(32, 64), (32, 64), (64, 32), (32, 32), (64, 64)]
    return [synthetic_view(k, h, w, win, SIZE) for k, ((h, w), win) in enumerate(zip(shapes, windows))], windows


@pytest.mark.parametrize("merger", ["median", "mean"])
def test_mirroring_every_map_and_toggling_every_flip_gives_the_same_merge(merger):
    """A view and its mirror image with x negated, marked as flipped, are the same statement about the image."""
    maps, windows = _small_case()
    base = merge_restatement(maps, windows, SIZE, merger, dtype=torch.float64)
    mirrored = []
    for m in maps:
        n = (2 * m.double() - 1).flip(-1)
        n[0] = -n[0]
        mirrored.append((n + 1) / 2)
    toggled = [(y0, x0, ch, cw, 1 - f) for y0, x0, ch, cw, f in windows]
    again = merge_restatement(mirrored, toggled, SIZE, merger, dtype=torch.float64)
    assert float((again - base).abs().max()) <= 1e-12


def test_one_whole_image_view_is_interpolate_and_normalise():
    m = synthetic_view(3, 32, 64, (0, 0, *SIZE, 0), SIZE)
    for merger in ("median", "mean"):
        got = merge_restatement([m], [(0, 0, *SIZE, 0)], SIZE, merger, normalize_views=False, dtype=torch.float64)
        v = F.interpolate(m.double()[None], SIZE, mode="bilinear", align_corners=False)[0]
        want = (F.normalize(2 * v - 1, dim=0) + 1) / 2
        assert float((got - want).abs().max()) <= 1e-12
        got = merge_restatement([m], [(0, 0, *SIZE, 0)], SIZE, merger, dtype=torch.float64)
        v = F.interpolate(F.normalize(2 * m.double() - 1, dim=0)[None], SIZE, mode="bilinear", align_corners=False)[0]
        assert float((got - (F.normalize(v, dim=0) + 1) / 2).abs().max()) <= 1e-12


def test_median_is_numpys_and_an_uncovered_pixel_is_the_zero_vector():
    flat = lambda v: torch.tensor(v, dtype=torch.float32).reshape(3, 1, 1).expand(3, 2, 2).contiguous()
    maps = [flat([0.9, 0.5, 0.9]), flat([0.6, 0.5, 0.8]), flat([0.7, 0.5, 0.7]), flat([0.2, 0.5, 1.0])]
    wins = [(0, 0, 2, 2, 0)] * 4
    got = merge_restatement(maps, wins, (2, 3), "median", normalize_views=False, dtype=torch.float64)
    n = torch.tensor([(0.6 + 0.7) - 1, 0.0, (0.8 + 0.9) - 1], dtype=torch.float64)      # the mean of the two middle values
    assert float((got[:, 0, 0] - (n / n.norm() + 1) / 2).abs().max()) <= 1e-7
    assert got[:, 0, 2].tolist() == [0.5, 0.5, 0.5]


# ------------------------------------------------------------------------------------------------ header and tables
def _header():
    return open(os.path.join(ROOT, "include", "dptx.h")).read()


def test_header_constants_and_struct_layout_match_the_ctypes_tables():
    text = _header()
    defines = {n: int(v) for n, v in re.findall(r"^#define (DPTX_\w+) (\d+)\s*$", text, flags=re.M)}
    assert defines["DPTX_TTA_MEAN"] == pp.TTA_MEAN == 32
    assert defines["DPTX_TTA_RAW_VIEWS"] == pp.TTA_RAW_VIEWS == 64
    assert defines["DPTX_TTA_MAX_VIEWS"] == pp.TTA_MAX_VIEWS == 64
    assert {k: defines["DPTX_RESIZE_" + k.upper()] for k in pp.RESIZE_MODES} == pp.RESIZE_MODES
    used = [pp.TTA_MEAN, pp.TTA_RAW_VIEWS, pp.RESIZE_RENORM]
    assert all(b & (b - 1) == 0 and b > max(pp.RESIZE_MODES.values()) for b in used) and len(set(used)) == 3
    body = re.search(r"typedef struct dptx_tta_view \{(.*?)\} dptx_tta_view;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(int64_t|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), C.c_int64 if ctype == "int64_t" else C.c_int32) for n in names.split(",")]
    assert fields == list(pp.TtaView._fields_)
    assert C.sizeof(pp.TtaView) == 40 and pp.TtaView.h.offset == 8 and pp.TtaView.flip.offset == 36


# ------------------------------------------------------------------------------------------------ argument checks
def _view(image=0, offset=0, h=64, w=96, y0=0, x0=0, ch=70, cw=93, flip=0):
    return pp.TtaView(offset, h, w, image, y0, x0, ch, cw, flip)


def _out(H=70, W=93, bpp=3, stride=None, offset=0):
    return pp.ImageDesc(offset, H, W, 3, W * bpp if stride is None else stride)


def _merge(lib, views, outs, mode=NORMAL_U8, n_views=None, B=None, maps=PTR, out=PTR, views_null=False, outs_null=False):
    va = (pp.TtaView * max(len(views), 1))(*views)
    oa = (pp.ImageDesc * max(len(outs), 1))(*outs)
    return lib.dptx_tta_merge_normals(maps, None if views_null else C.addressof(va), len(views) if n_views is None else n_views,
                                      None if outs_null else C.addressof(oa), len(outs) if B is None else B, mode, out, None)


def test_merge_rejects_bad_arguments_without_a_gpu(lib):
    u8, f32 = _out(), _out(bpp=4)
    assert _merge(lib, [_view()] * 65, [u8]) == INVALID                                   # 65 views for one image
    assert _merge(lib, [_view()] * 64 + [_view(image=1)] * 65, [u8, u8]) == INVALID
    assert _merge(lib, [_view(y0=1)], [u8]) == INVALID                                    # a window outside the image
    assert _merge(lib, [_view(x0=1)], [u8]) == INVALID
    assert _merge(lib, [_view(y0=-1, ch=10)], [u8]) == INVALID
    assert _merge(lib, [_view(ch=0)], [u8]) == INVALID
    assert _merge(lib, [_view(cw=94)], [u8]) == INVALID
    assert _merge(lib, [_view(), _view(image=1, ch=40, cw=50)], [u8, _out(H=40, W=49)]) == INVALID
    assert _merge(lib, [_view(), _view(image=1), _view()], [u8, u8]) == INVALID           # views not grouped by image
    assert _merge(lib, [_view(image=1), _view()], [u8, u8]) == INVALID                    # images not ascending
    assert _merge(lib, [_view(), _view(image=2)], [u8, u8, u8]) == INVALID                # an image without a view
    assert _merge(lib, [_view(), _view()], [u8, u8]) == INVALID
    assert _merge(lib, [_view(image=1)], [u8]) == INVALID
    assert _merge(lib, [_view(image=-1)], [u8]) == INVALID
    assert _merge(lib, [_view(offset=2)], [u8]) == INVALID                                # a misaligned offset
    assert _merge(lib, [_view(offset=-4)], [u8]) == INVALID
    assert _merge(lib, [_view()], [u8], maps=PTR + 2) == INVALID
    assert _merge(lib, [_view()], [_out(bpp=4, stride=93 * 4 + 2)], NORMAL_F32) == INVALID  # fp32 mode, unaligned stride
    assert _merge(lib, [_view()], [_out(bpp=4, offset=2)], NORMAL_F32) == INVALID
    assert _merge(lib, [_view()], [f32], NORMAL_F32, out=PTR + 1) == INVALID
    assert _merge(lib, [_view()], [_out(stride=93 * 3 - 1)]) == INVALID
    assert _merge(lib, [_view()], [_out(stride=93 * 4 - 4, bpp=4)], NORMAL_F32) == INVALID
    assert _merge(lib, [_view()], [u8], B=0) == INVALID                                   # B or n_views of 0
    assert _merge(lib, [_view()], [u8], n_views=0) == INVALID
    assert _merge(lib, [_view()], [u8], B=4097) == INVALID
    assert _merge(lib, [_view(h=0)], [u8]) == INVALID
    assert _merge(lib, [_view(w=4097)], [u8]) == INVALID
    assert _merge(lib, [_view(ch=16385)], [_out(H=16385)]) == INVALID
    for mode in (0, DEPTH_F32, 4, NORMAL_U8 | RENORM, NORMAL_F32 | 128, NORMAL_U8 | 8, pp.TTA_MEAN, pp.TTA_RAW_VIEWS, -1):
        assert _merge(lib, [_view()], [f32], mode) == INVALID                             # unknown mode
    assert _merge(lib, [_view()], [u8], maps=None) == INVALID
    assert _merge(lib, [_view()], [u8], out=None) == INVALID
    assert _merge(lib, [_view()], [u8], views_null=True) == INVALID
    assert _merge(lib, [_view()], [u8], outs_null=True) == INVALID


def test_views_preprocess_rejects_what_the_rect_entry_rejects_without_a_gpu(lib):
    def pre(descs, B=None, OH=64, OW=96, pixels=PTR, x=PTR, ws=PTR, ws_bytes=1 << 40, flips=(), descs_null=False):
        arr = (pp.ImageDesc * max(len(descs), 1))(*descs)
        fl = (C.c_uint8 * max(len(flips), 1))(*flips)
        return lib.dptx_preprocess_u8_views_batch(pixels, None if descs_null else C.addressof(arr), C.addressof(fl) if flips else None,
                                                  len(descs) if B is None else B, OH, OW, 0, x, ws, ws_bytes, None)
    good = pp.ImageDesc(0, 70, 90, 3, 270)
    window = pp.window_desc(good, (10, 5, 80, 60))
    assert (window.offset, window.H, window.W, window.C, window.row_stride_bytes) == (5 * 270 + 30, 55, 70, 3, 270)
    with pytest.raises(ValueError):
        pp.window_desc(good, (10, 5, 91, 60))
    assert pre([good], B=0) == INVALID
    assert pre([good, window], B=4097, flips=(0, 1)) == INVALID
    assert pre([good], OH=48) == INVALID
    assert pre([good], OW=1056) == INVALID
    assert pre([pp.ImageDesc(0, 32 * 64 + 1, 90, 3, 270)]) == INVALID
    assert pre([pp.ImageDesc(0, 70, 90, 2, 270)], flips=(1,)) == INVALID
    assert pre([pp.ImageDesc(0, 70, 90, 3, 269)]) == INVALID
    assert pre([good, pp.ImageDesc(-16, 70, 90, 3, 270)], flips=(1, 0)) == INVALID
    assert pre([good], pixels=None) == INVALID
    assert pre([good], x=None) == INVALID
    assert pre([good], ws=None) == INVALID
    assert pre([good], descs_null=True) == INVALID
    assert pre([good], ws_bytes=8832 * 160 - 1) == INVALID
