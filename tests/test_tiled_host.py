"""Host side of tiled inference (omnidata_amd/tiled.py, csrc/tiles.hip): the planner's invariants, the restatement's own
conditions (the seam condition and the planted case), the header against the library, the argument checks of the four entry
points (they return before anything touches a GPU), and the argument rules of BatchPredictor and demo.py."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from omnidata_amd import preprocess as pp
from omnidata_amd import tiled
from tiled_restatement import (GRID, SIZE, blend_depth_restatement, blend_normals_restatement, crops_of, depth_reference,
                               normal_reference, planted_case, seam_case, starts, to_u8, u8_differences)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
PTR = 0x10000   # a non-null "device pointer": an argument check must reject the call before it is ever used
NORMAL_U8, NORMAL_F32, DEPTH_F32, DEPTH_RGBA, RENORM = 1, 2, 3, 4, 16
# (w, h): the sizes the definitions name, a window smaller than the tile on one or both axes, one pixel more than a tile, a strip
NINE_SIZES = [(683, 512), (4000, 3000), (16384, 16384), (384, 384), (100, 80), (385, 384), (1, 1000), (6000, 4000), (1024, 300)]


@pytest.fixture(scope="module")
def lib(built_lib):
    from omnidata_amd.engine import load_library
    return load_library()


# ------------------------------------------------------------------------------------------------ planner
@pytest.mark.parametrize("w,h", NINE_SIZES)
def test_planner_invariants(w, h):
    p = tiled.plan_tiles(w, h)
    (ch, cw), (ry, rx) = p.window, p.ramps
    assert (ch, cw) == (min(h, 384), min(w, 384))
    assert (ry, rx) == (min(int(0.25 * ch + 0.5), ch // 2), min(int(0.25 * cw + 0.5), cw // 2))
    for s, c, r, L in ((p.ys, ch, ry, h), (p.xs, cw, rx, w)):
        assert s[0] == 0 and s[-1] + c == L and s == starts(L, c, r) and 1 <= len(s) <= 64
        assert all(b > a and a + c - b >= r for a, b in zip(s, s[1:]))                   # ascending, overlap at least the ramp
        assert len(s) == (1 if c == L else math.ceil((L - r) / (c - r)))
    assert all(v % 32 == 0 and 32 <= v <= 1024 for v in p.net + p.anchor_net)
    if ch == cw:
        assert p.net == (384, 384)
    aw, ah, _ = pp.full_frame_net_size(w, h, 384, 32)
    assert p.anchor_net == (ah, aw)


def test_planner_grids_of_the_named_sizes_the_cap_and_the_options():
    assert tiled.plan_tiles(683, 512).xs == [0, 150, 299] and tiled.plan_tiles(683, 512).ys == [0, 128]
    p = tiled.plan_tiles(4000, 3000)
    assert (len(p.xs), len(p.ys)) == (14, 11)
    p = tiled.plan_tiles(16384, 16384)
    assert (len(p.xs), len(p.ys)) == (57, 57)
    with pytest.raises(ValueError, match="at most 64"):
        tiled.plan_tiles(16384, 16384, tile=128)                                          # 171 starts per axis
    with pytest.raises(ValueError, match="at most 64"):
        tiled.plan_tiles(16384, 300, scale=0.5)
    for bad in (dict(overlap=-0.01), dict(overlap=0.51), dict(tile=0), dict(scale=0.0)):
        with pytest.raises(ValueError):
            tiled.plan_tiles(640, 480, **bad)
    p = tiled.plan_tiles(1000, 800, tile=384, scale=2.0)                                  # 768-pixel windows at 384 network pixels
    assert p.window == (768, 768) and p.net == (384, 384) and p.ramps == (192, 192)
    p = tiled.plan_tiles(1000, 800, overlap=0.0)
    assert p.ramps == (0, 0) and p.xs == [0, 308, 616] and p.ys == [0, 208, 416]
    p = tiled.plan_tiles(2000, 300, multiple=64, max_side=512)                            # the version-1 UNet's sizes
    assert p.window == (300, 384) and p.net == (384, 512) and p.anchor_net == (384, 512)
    assert p.net[0] % 64 == 0 and p.net[1] % 64 == 0


# ------------------------------------------------------------------------------------------------ the restatement's own conditions
def test_seam_condition_tiles_that_are_exact_crops_blend_back_to_the_map():
    depth, normals = seam_case()
    for dtype in (torch.float32, torch.float64):
        out, _ = blend_depth_restatement(crops_of(depth, GRID), GRID, SIZE, None, dtype, align=False)
        err_d = float((out.double() - (1 - depth.double())).abs().max())
        got = blend_normals_restatement(crops_of(normals, GRID), GRID, SIZE, dtype, normalize_views=False)
        err_n = float((got.double() - normals.double()).abs().max())
        print(f"seam condition {dtype}: depth {err_d:.3e} normals {err_n:.3e}")
        assert err_d <= 1e-6 and err_n <= 1e-6


def test_planted_case_aligned_recovers_the_truth_and_unaligned_does_not():
    maps, anchor, tr = planted_case()
    for dtype in (torch.float32, torch.float64):
        aligned, coeffs = blend_depth_restatement(maps, GRID, SIZE, anchor, dtype)
        plain, _ = blend_depth_restatement(maps, GRID, SIZE, None, dtype, align=False)
        e_a, e_p = float(((1 - aligned.double()) - tr).abs().max()), float(((1 - plain.double()) - tr).abs().max())
        print(f"planted case {dtype}: aligned {e_a:.3e} unaligned {e_p:.3e}")
        assert e_a <= 1e-5 and e_p >= 1e-2
        assert coeffs.shape == (9, 2)


def test_the_fp32_restatement_meets_the_uint8_cap_against_the_fp64_one():
    o64, o32, e_ref = normal_reference()
    worst, frac = u8_differences(to_u8(o32), to_u8(o64))
    print(f"uint8 fp32 vs fp64 restatement: e_ref {e_ref:.3e}, worst {worst} level(s), {frac:.2e} of the bytes differ")
    assert worst <= 1 and frac <= 0.01
    _, _, e_ref_d, e_ref_c = depth_reference()
    assert e_ref <= 1e-5 and e_ref_d <= 1e-5 and e_ref_c <= 1e-3


# ------------------------------------------------------------------------------------------------ header
def test_header_declares_the_entry_points_and_the_library_exports_them(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dptx.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", text)
    for proto in ("int dptx_tile_blend_normals(const void* views_dev, const dptx_tile_grid* grids, const dptx_image_desc* outs, "
                  "int32_t B, int32_t mode, void* out_dev, void* stream);",
                  "int dptx_tile_depth_workspace_bytes(const dptx_tile_grid* grids, const dptx_image_desc* outs, int32_t B, "
                  "int64_t* bytes);",
                  "int dptx_tile_align_depth(const void* views_dev, const dptx_tile_grid* grids, const dptx_image_desc* outs, "
                  "int32_t B, float* coeffs_dev, void* ws, int64_t ws_bytes, void* stream);",
                  "int dptx_tile_blend_depth(const void* views_dev, const dptx_tile_grid* grids, const float* coeffs_dev, "
                  "const dptx_image_desc* outs, int32_t B, int32_t mode, void* out_dev, void* stream);"):
        assert proto in flat, proto
    defines = {n: int(v) for n, v in re.findall(r"^#define (DPTX_\w+) (\d+)\s*$", text, flags=re.M)}
    assert defines["DPTX_TILE_MAX_AXIS"] == pp.TILE_MAX_AXIS == 64
    assert C.sizeof(pp.TileGrid) == 8 + 8 + 10 * 4 + 2 * 64 * 4                          # the struct of the header, no padding
    for name in ("dptx_tile_blend_normals", "dptx_tile_depth_workspace_bytes", "dptx_tile_align_depth", "dptx_tile_blend_depth"):
        assert hasattr(lib, name)
    from omnidata_amd.build import HEADERS, SOURCE_FLAGS, SOURCES
    assert "tiles.hip" in SOURCES and "tta_depth_align.h" in HEADERS and "-packed-fp32-ops" in SOURCE_FLAGS["tiles.hip"]
    assert "plan_tiles" in tiled.__doc__ and "fminf" in open(os.path.join(ROOT, "include", "dptx.h")).read()


# ------------------------------------------------------------------------------------------------ argument checks
def _grid(offset=0, anchor_offset=0, h=32, w=32, ch=48, cw=64, ys=(0, 25, 49), xs=(0, 43, 86), ry=12, rx=16, ah=40, aw=56,
          ny=None, nx=None):
    g = pp.TileGrid.make(offset, (h, w), (ch, cw), ys, xs, (ry, rx), anchor_offset, (ah, aw))
    if ny is not None:
        g.ny = ny
    if nx is not None:
        g.nx = nx
    return g


def _out(H=97, W=150, stride=None, offset=0, bpp=4):
    return pp.ImageDesc(offset, H, W, 1, W * bpp if stride is None else stride)


def _calls(lib, grids, outs, B=None, maps=PTR, out=PTR, coeffs=PTR, ws=PTR, ws_bytes=1 << 40, mode_n=NORMAL_F32, mode_d=DEPTH_F32,
           grids_null=False, outs_null=False):
    """-> the return codes of (blend_normals, workspace_bytes, align, blend_depth) for one set of arguments"""
    ga = (pp.TileGrid * max(len(grids), 1))(*grids)
    oa = (pp.ImageDesc * max(len(outs), 1))(*outs)
    gp, op = None if grids_null else C.addressof(ga), None if outs_null else C.addressof(oa)
    nb = len(outs) if B is None else B
    nbytes = C.c_int64(-1)
    return (lib.dptx_tile_blend_normals(maps, gp, op, nb, mode_n, out, None),
            lib.dptx_tile_depth_workspace_bytes(gp, op, nb, C.byref(nbytes)),
            lib.dptx_tile_align_depth(maps, gp, op, nb, coeffs, ws, ws_bytes, None),
            lib.dptx_tile_blend_depth(maps, gp, coeffs, op, nb, mode_d, out, None))


def test_the_four_entry_points_reject_bad_arguments_without_a_gpu(lib):
    good, grid = _out(), _grid()
    every = (INVALID,) * 4
    # the grid: starts ascending from 0, no gap, the last window ends at the image's edge
    assert _calls(lib, [_grid(ys=(0, 49, 25))], [good]) == every                           # not ascending
    assert _calls(lib, [_grid(xs=(0, 43, 43, 86))], [good]) == every                       # a start twice
    assert _calls(lib, [_grid(ys=(0, 49))], [good]) == every                               # a gap: row 48 is in no window
    assert _calls(lib, [_grid(xs=(0, 86))], [good]) == every
    assert _calls(lib, [_grid(ys=(1, 25, 49))], [good]) == every                           # the first start is not 0
    assert _calls(lib, [_grid(ys=(0, 25, 48))], [good]) == every                           # the last window ends short of H
    assert _calls(lib, [_grid(xs=(0, 43, 87))], [good]) == every                           # a window outside the image
    assert _calls(lib, [_grid(ys=(0, 25, 50))], [good]) == every
    assert _calls(lib, [_grid(ch=98, ys=(0,))], [good]) == every                           # a window larger than the image
    assert _calls(lib, [_grid(ch=0)], [good]) == every
    assert _calls(lib, [_grid(cw=-1)], [good]) == every
    for n in (0, 65, -1):
        assert _calls(lib, [_grid(ny=n)], [good]) == every                                 # ny / nx outside 1..64
        assert _calls(lib, [_grid(nx=n)], [good]) == every
    assert _calls(lib, [_grid(ry=-1)], [good]) == every
    assert _calls(lib, [_grid(rx=-1)], [good]) == every
    # the ranges of dptx_tta_merge_normals
    assert _calls(lib, [_grid(offset=2)], [good]) == every                                 # a misaligned offset
    assert _calls(lib, [_grid(offset=-4)], [good]) == every
    assert _calls(lib, [_grid(h=0)], [good]) == every
    assert _calls(lib, [_grid(w=4097)], [good]) == every
    assert _calls(lib, [grid], [_out(H=16385)]) == every
    assert _calls(lib, [grid], [_out(stride=150 * 4 - 4)]) == every
    assert _calls(lib, [grid], [_out(offset=-4)]) == every
    assert _calls(lib, [grid], [good], B=0) == every
    assert _calls(lib, [grid], [good], B=4097) == every
    assert _calls(lib, [grid], [good], grids_null=True) == every
    assert _calls(lib, [grid], [good], outs_null=True) == every
    assert _calls(lib, [grid, _grid(ys=(0, 49))], [good, good]) == every                   # the second image's grid
    # fp32 rows: stride and offset in dwords (the normals call is asked for fp32 here too)
    assert _calls(lib, [grid], [_out(stride=150 * 4 + 2)]) == every
    assert _calls(lib, [grid], [_out(offset=2)]) == every
    # device pointers
    assert _calls(lib, [grid], [good], maps=None)[0::2] == (INVALID, INVALID) and _calls(lib, [grid], [good], maps=None)[3] == INVALID
    assert _calls(lib, [grid], [good], maps=PTR + 2)[0::2] == (INVALID, INVALID) and _calls(lib, [grid], [good], maps=PTR + 2)[3] == INVALID
    assert _calls(lib, [grid], [good], out=None)[0::3] == (INVALID, INVALID)
    assert _calls(lib, [grid], [good], out=PTR + 1)[0::3] == (INVALID, INVALID)
    assert _calls(lib, [grid], [good], coeffs=PTR + 2)[2:] == (INVALID, INVALID)
    assert _calls(lib, [grid], [good], coeffs=None)[2] == INVALID                          # align has to write them
    assert _calls(lib, [grid], [good], ws=None)[2] == INVALID
    assert _calls(lib, [grid], [good], ws=PTR + 4)[2] == INVALID
    # the anchor: the alignment needs one
    assert _calls(lib, [_grid(anchor_offset=-1)], [good])[2] == INVALID
    assert _calls(lib, [_grid(anchor_offset=2)], [good])[2] == INVALID
    assert _calls(lib, [_grid(ah=0)], [good])[2] == INVALID
    assert _calls(lib, [_grid(aw=4097)], [good])[2] == INVALID
    # the workspace: exactly what the host-only entry asks for -- the plane, and the records of one chunk of at most 63 tiles
    ga, oa, nbytes = (pp.TileGrid * 1)(grid), (pp.ImageDesc * 1)(good), C.c_int64()
    assert lib.dptx_tile_depth_workspace_bytes(C.addressof(ga), C.addressof(oa), 1, C.byref(nbytes)) == 0
    plane = (97 * 150 * 4 + 255) // 256 * 256
    assert nbytes.value == plane + (9 * 3 * 32 + 255) // 256 * 256                         # 9 tiles, 1 x 3 stats tiles of a 48 x 64 window
    assert lib.dptx_tile_depth_workspace_bytes(C.addressof(ga), C.addressof(oa), 1, None) == INVALID
    assert _calls(lib, [grid], [good], ws_bytes=nbytes.value - 1)[2] == INVALID
    many = _grid(ch=8, cw=8, ys=range(0, 253, 4), xs=range(0, 253, 4), ry=4, rx=4)
    ga, oa = (pp.TileGrid * 1)(many), (pp.ImageDesc * 1)(_out(260, 260))
    assert lib.dptx_tile_depth_workspace_bytes(C.addressof(ga), C.addressof(oa), 1, C.byref(nbytes)) == 0
    assert nbytes.value == (260 * 260 * 4 + 255) // 256 * 256 + (63 * 32 + 255) // 256 * 256
    # the modes: normals U8 / F32, | DPTX_TTA_RAW_VIEWS; depth F32; nothing else
    for mode in (0, DEPTH_F32, DEPTH_RGBA, NORMAL_F32 | RENORM, NORMAL_F32 | pp.TTA_MEAN, NORMAL_U8 | 128, pp.TTA_RAW_VIEWS, -1):
        assert _calls(lib, [grid], [good], mode_n=mode)[0] == INVALID
    for mode in (0, NORMAL_U8, NORMAL_F32, DEPTH_RGBA, DEPTH_F32 | RENORM, DEPTH_F32 | pp.TTA_MEAN, DEPTH_F32 | pp.TTA_RAW_VIEWS, -1):
        assert _calls(lib, [grid], [good], mode_d=mode)[3] == INVALID
    # uint8 rows may start at any byte, but must hold the row
    oa = (pp.ImageDesc * 1)(_out(stride=150 * 3 - 1, bpp=3))
    assert lib.dptx_tile_blend_normals(PTR, C.addressof(ga), C.addressof(oa), 1, NORMAL_U8, PTR, None) == INVALID


# ------------------------------------------------------------------------------------------------ argument rules above the library
class _NoModel:
    """Stands where a model goes: every rule below must be decided before the model is touched."""

    def parameters(self):
        raise AssertionError("the model was touched before the arguments were checked")


def test_batch_predictor_and_class_argument_rules():
    from omnidata_amd.batch_infer import BatchPredictor
    model = _NoModel()
    with pytest.raises(ValueError, match="tiled excludes"):
        BatchPredictor(model, "normal", tiled=True, tta="flip")
    with pytest.raises(ValueError, match="tiled excludes"):
        BatchPredictor(model, "depth", tiled={"tile": 64}, tta="flip", tta_align="lstsq")
    with pytest.raises(ValueError, match="tiled excludes"):
        BatchPredictor(model, "normal", tiled=True, full_frame="aspect")
    with pytest.raises(ValueError, match="tiled must be"):
        BatchPredictor(model, "normal", tiled="yes")
    with pytest.raises(ValueError, match="DPT depth model"):
        tiled.TiledDepth(model)
    for kw in (dict(overlap=0.6), dict(batch_size=0), dict(chunk_images=0), dict(tile=0)):
        with pytest.raises(ValueError):
            tiled.TiledNormals(model, **kw)
    with pytest.raises(ValueError):
        tiled.TiledDepth(model, align="affine")


@pytest.mark.parametrize("argv,message", [
    (["--task", "normal", "--tiled", "--tta", "flip"], "--tiled excludes --full_frame and --tta"),
    (["--task", "depth", "--tiled", "--full_frame", "aspect"], "--tiled excludes --full_frame and --tta"),
    (["--task", "normal", "--tiled", "--tile_overlap", "0.7"], "--tile_overlap in [0, 0.5]"),
    (["--task", "depth", "--tiled", "--backbone", "unet"], "--backbone unet --task depth has no --tiled"),
])
def test_demo_cli_refuses_before_it_builds_a_model(argv, message, tmp_path, capsys, monkeypatch):
    monkeypatch.syspath_prepend(ROOT)
    import demo
    with pytest.raises(SystemExit):
        demo.main(argv + ["--img_path", str(tmp_path), "--output_path", str(tmp_path / "out")])
    assert message in capsys.readouterr().out
    assert not (tmp_path / "out").exists()
