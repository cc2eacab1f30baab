"""Host side of full-frame inference (csrc/fullframe.hip, omnidata_amd/preprocess.py, omnidata_amd/batch_infer.py): the network
size rule against the reference's table, the bucketing plan, and the argument checks of the two entry points (they return
before anything touches a GPU)."""
import ctypes as C
import json
import os

import pytest

from omnidata_amd import preprocess as pp
from omnidata_amd.batch_infer import plan_full_frame

INVALID = -1
PTR = 0x10000   # a non-null "device pointer": an argument check must reject the call before it is ever used
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fullframe_sizes.json")
NORMAL_U8, NORMAL_F32, DEPTH_F32, DEPTH_RGBA, RENORM = 1, 2, 3, 4, 16


@pytest.fixture(scope="module")
def lib(built_lib):
    from omnidata_amd.engine import load_library
    return load_library()


def test_full_frame_size_equals_every_row_of_the_references_table():
    table = json.load(open(GOLDEN))
    assert table["columns"] == ["w", "h", "size", "multiple", "net_w", "net_h"]
    rows = [tuple(r) for r in table["rows"]]
    assert len(rows) >= 300
    assert {(384, 32), (64, 32), (384, 64)} <= {r[2:4] for r in rows}
    for want in [(640, 512, 384, 32, 480, 384), (1920, 1080, 384, 32, 672, 384), (4000, 3000, 384, 32, 512, 384),
                 (3000, 4000, 384, 32, 384, 512), (400, 400, 384, 32, 384, 384), (777, 385, 384, 32, 768, 384),
                 (50, 33, 384, 32, 576, 384), (2048, 640, 384, 32, 1216, 384), (1000, 999, 384, 32, 384, 384),
                 (1039, 640, 384, 32, 608, 384)]:
        assert want in rows
    for w, h, size, multiple, nw, nh in rows:
        assert pp.full_frame_size(w, h, size, multiple) == (nw, nh), (w, h, size, multiple)
    assert pp.full_frame_size(1920, 1080) == (672, 384)     # the defaults: size 384, multiple 32


def test_net_size_caps_the_long_side_and_says_so():
    assert pp.full_frame_net_size(1920, 1080) == (672, 384, False)
    assert pp.full_frame_net_size(2048, 640) == (1024, 384, True)        # 1216 -> 1024
    assert pp.full_frame_net_size(100, 4000) == (384, 1024, True)
    for w, h in ((50, 33), (16384, 100), (3, 16000), (5000, 5000)):
        nw, nh, _ = pp.full_frame_net_size(w, h)
        assert nw % 32 == 0 and nh % 32 == 0 and 384 <= nw <= 1024 and 384 <= nh <= 1024 and nw * nh * 256 < 2 ** 31


def test_bucketing_restores_the_order_puts_the_largest_shape_first_and_caps():
    sizes = [(90, 70), (70, 90), (64, 64), (50, 33), (300, 120), (91, 70), (1000, 10)]    # (w, h)
    chunks, capped = plan_full_frame(sizes, "aspect", image_size=64, batch_size=2)
    nets = [net for net, _ in chunks]
    areas = [nh * nw for nh, nw in nets]
    assert areas == sorted(areas, reverse=True)                                             # the arena is planned once
    assert nets[0] == (64, 1024) and capped == [6]                                          # 6400 wide -> cut back, and reported
    for (nh, nw), idxs in chunks:
        assert 1 <= len(idxs) <= 2 and idxs == sorted(idxs)
        for i in idxs:
            w, h = sizes[i]
            assert (nw, nh) == pp.full_frame_net_size(w, h, 64)[:2]
    assert sorted(i for _, idxs in chunks for i in idxs) == list(range(len(sizes)))        # every input exactly once
    by_net = {}
    for net, idxs in chunks:
        by_net.setdefault(net, []).extend(idxs)
    assert by_net[(64, 96)] == [0, 3, 5]                                                    # 90x70, 50x33 and 91x70 share a shape
    assert [len(idxs) for net, idxs in chunks if net == (64, 96)] == [2, 1]
    # squash: one shape, batching as without full_frame
    chunks, capped = plan_full_frame(sizes, "squash", image_size=64, batch_size=3)
    assert capped == [] and chunks == [((64, 64), [0, 1, 2]), ((64, 64), [3, 4, 5]), ((64, 64), [6])]
    assert plan_full_frame([], "aspect") == ([], [])
    with pytest.raises(ValueError):
        plan_full_frame(sizes, "crop")


def _desc(H=70, W=90, Cn=3, stride=None, offset=0, bpp=None):
    return pp.ImageDesc(offset, H, W, Cn, W * (Cn if bpp is None else bpp) if stride is None else stride)


def _pre(lib, descs, B=None, OH=64, OW=96, pixels=PTR, x=PTR, ws=PTR, ws_bytes=1 << 40, descs_null=False):
    arr = (pp.ImageDesc * max(len(descs), 1))(*descs)
    return lib.dptx_preprocess_u8_rect_batch(pixels, None if descs_null else C.addressof(arr), len(descs) if B is None else B, OH, OW,
                                             0, x, ws, ws_bytes, None)


def test_rect_preprocess_rejects_bad_arguments_without_a_gpu(lib):
    good = _desc()
    assert _pre(lib, [good], B=0) == INVALID
    assert _pre(lib, [good], B=4097) == INVALID
    assert _pre(lib, [good], OH=48) == INVALID                                  # not a multiple of 32
    assert _pre(lib, [good], OW=100) == INVALID
    assert _pre(lib, [good], OH=32) == INVALID                                  # below 64
    assert _pre(lib, [good], OW=1056) == INVALID
    assert _pre(lib, [_desc(H=32 * 64 + 1, W=90)]) == INVALID                   # H > 32 * OH
    assert _pre(lib, [_desc(H=70, W=32 * 96 + 1)]) == INVALID                   # W > 32 * OW
    assert _pre(lib, [_desc(Cn=2)]) == INVALID
    assert _pre(lib, [_desc(stride=90 * 3 - 1)]) == INVALID
    assert _pre(lib, [_desc(H=0)]) == INVALID
    assert _pre(lib, [_desc(W=16385, H=64)], OW=1024) == INVALID
    assert _pre(lib, [_desc(offset=-16)]) == INVALID
    assert _pre(lib, [good, _desc(Cn=2)]) == INVALID                            # any image of the batch
    assert _pre(lib, [good], pixels=None) == INVALID
    assert _pre(lib, [good], x=None) == INVALID
    assert _pre(lib, [good], ws=None) == INVALID
    assert _pre(lib, [good], descs_null=True) == INVALID
    assert _pre(lib, [good], ws_bytes=8832 * 160 - 1) == INVALID                # smaller than the workspace it reports


def _post(lib, descs, mode, B=None, Cn=None, h=64, w=96, y=PTR, out=PTR, lut=PTR, ws=PTR, ws_bytes=1 << 40, descs_null=False):
    arr = (pp.ImageDesc * max(len(descs), 1))(*descs)
    if Cn is None:
        Cn = 3 if (mode & 15) in (NORMAL_U8, NORMAL_F32) else 1
    return lib.dptx_postprocess_resize_batch(y, len(descs) if B is None else B, Cn, h, w, None if descs_null else C.addressof(arr),
                                             mode, out, lut, ws, ws_bytes, None)


def test_resize_outputs_rejects_bad_arguments_without_a_gpu(lib):
    u8, f32 = _desc(bpp=3), _desc(bpp=4)
    assert _post(lib, [u8], NORMAL_U8, B=0) == INVALID
    assert _post(lib, [u8], NORMAL_U8, B=4097) == INVALID
    for mode in (0, 5, 15, RENORM, NORMAL_U8 | 32, DEPTH_F32 | RENORM, DEPTH_RGBA | RENORM, -1):
        assert _post(lib, [f32], mode, Cn=3) == INVALID and _post(lib, [f32], mode, Cn=1) == INVALID     # unknown mode
    assert _post(lib, [_desc(stride=90 * 3 - 1)], NORMAL_U8) == INVALID         # row_stride_bytes < W * bytes per pixel
    assert _post(lib, [_desc(stride=90 * 4 - 4)], NORMAL_F32) == INVALID
    assert _post(lib, [_desc(stride=90 * 4 - 4)], DEPTH_F32) == INVALID
    assert _post(lib, [_desc(stride=90 * 4 - 4)], DEPTH_RGBA) == INVALID
    assert _post(lib, [_desc(stride=90 * 4 + 2)], DEPTH_F32) == INVALID         # dword stores: stride and offset multiples of 4
    assert _post(lib, [_desc(bpp=4, offset=2)], NORMAL_F32) == INVALID
    assert _post(lib, [u8], NORMAL_U8, Cn=1) == INVALID                         # channels and mode disagree
    assert _post(lib, [f32], DEPTH_F32, Cn=3) == INVALID
    assert _post(lib, [u8], NORMAL_U8, h=0) == INVALID
    assert _post(lib, [u8], NORMAL_U8, w=4097) == INVALID
    assert _post(lib, [_desc(H=0, bpp=3)], NORMAL_U8) == INVALID
    assert _post(lib, [_desc(W=16385, bpp=3)], NORMAL_U8) == INVALID
    assert _post(lib, [_desc(bpp=3, offset=-1)], NORMAL_U8) == INVALID
    assert _post(lib, [u8, _desc(stride=1)], NORMAL_U8) == INVALID              # any output of the batch
    assert _post(lib, [u8], NORMAL_U8, y=None) == INVALID
    assert _post(lib, [u8], NORMAL_U8, out=None) == INVALID
    assert _post(lib, [u8], NORMAL_U8, descs_null=True) == INVALID
    assert _post(lib, [f32], DEPTH_RGBA, lut=None) == INVALID                   # the colormap and the workspace: DEPTH_RGBA only
    assert _post(lib, [f32], DEPTH_RGBA, ws=None) == INVALID
    assert _post(lib, [f32], DEPTH_RGBA, ws_bytes=16383) == INVALID


def test_workspace_sizes_are_reported_on_the_host(lib):
    n = C.c_int64()
    pre = lib.dptx_preprocess_rect_batch_workspace_bytes
    assert pre(1, 64, 96, C.byref(n)) == 0 and n.value == 8832 * 160
    assert pre(4096, 384, 672, C.byref(n)) == 0 and n.value == 8832 * (384 + 672)
    sq = C.c_int64()
    assert lib.dptx_preprocess_batch_workspace_bytes(1, 384, C.byref(sq)) == 0
    assert pre(1, 384, 384, C.byref(n)) == 0 and n.value == sq.value            # a square target: the square entry's layout
    for B, OH, OW in ((0, 64, 64), (4097, 64, 64), (1, 48, 64), (1, 64, 48), (1, 32, 64), (1, 64, 1056), (1, 2048, 64)):
        assert pre(B, OH, OW, C.byref(n)) == INVALID
    assert pre(1, 64, 64, None) == INVALID
    post = lib.dptx_postprocess_resize_workspace_bytes
    for mode in (NORMAL_U8, NORMAL_F32, DEPTH_F32, NORMAL_U8 | RENORM, NORMAL_F32 | RENORM):
        assert post(33, mode, C.byref(n)) == 0 and n.value == 0
    assert post(1, DEPTH_RGBA, C.byref(n)) == 0 and n.value == 16384
    assert post(4096, DEPTH_RGBA, C.byref(n)) == 0 and n.value == 16384          # 32 images x 64 (min, max) pairs, whatever B is
    for B, mode in ((0, NORMAL_U8), (4097, NORMAL_U8), (1, 0), (1, 5), (1, DEPTH_F32 | RENORM), (1, RENORM)):
        assert post(B, mode, C.byref(n)) == INVALID
    assert post(1, NORMAL_U8, None) == INVALID
