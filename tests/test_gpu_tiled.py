"""Tiled inference on the GPU (csrc/tiles.hip, omnidata_amd/tiled.py): the blends and the alignment against their restatement
(tests/tiled_restatement.py; the cases and bounds of tests/tiled_checks.py, which the host build under the sanitizers runs too),
the cross-checks against the TTA entry points bit for bit, and the pipeline end to end.  pytest -m gpu.

Measured on an MI355X: profiles/tiled_parity.md."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from omnidata_amd import preprocess as pp
from omnidata_amd import tiled
import tiled_checks as checks
from tiled_restatement import CASES, case_maps, pack_tiles

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class GpuRunner:
    """tiled_checks' runner over the library's entry points: raw buffers, filled with 0xA5 before the call."""

    def __init__(self):
        from omnidata_amd.engine import load_library
        self.lib = load_library()

    @staticmethod
    def _args(flat, grids, total):
        dev = flat.to(DEV)
        out = torch.full((total,), checks.FILL, dtype=torch.uint8, device=DEV)
        return dev, (pp.TileGrid * len(grids))(*grids), out, torch.cuda.current_stream().cuda_stream

    def normals(self, flat, grids, descs, total, mode):
        dev, arr, out, stream = self._args(flat, grids, total)
        assert self.lib.dptx_tile_blend_normals(dev.data_ptr(), C.addressof(arr), C.addressof(descs), len(grids), mode, out.data_ptr(),
                                                stream) == 0
        return out.cpu()

    def depth(self, flat, grids, descs, total, align):
        dev, arr, out, stream = self._args(flat, grids, total)
        coeffs = torch.full((sum(g.tiles for g in grids), 2), float("nan"), dtype=torch.float32, device=DEV)
        if align:
            nbytes = C.c_int64()
            assert self.lib.dptx_tile_depth_workspace_bytes(C.addressof(arr), C.addressof(descs), len(grids), C.byref(nbytes)) == 0
            ws = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device=DEV)        # NaN records
            assert self.lib.dptx_tile_align_depth(dev.data_ptr(), C.addressof(arr), C.addressof(descs), len(grids), coeffs.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), stream) == 0
        assert self.lib.dptx_tile_blend_depth(dev.data_ptr(), C.addressof(arr), coeffs.data_ptr() if align else None, C.addressof(descs),
                                              len(grids), checks.DEPTH_F32, out.data_ptr(), stream) == 0
        return out.cpu(), coeffs.cpu()


@pytest.fixture(scope="module")
def R():
    return GpuRunner()


# ------------------------------------------------------------------------------------------------ against the restatement
def test_normals_depth_and_coefficients_within_twice_the_restatements_own_rounding_and_uint8_within_a_level(R):
    """150 x 97, 3 x 3 tiles, maps of 32 x 32 for windows of 64 x 48: err <= 2 e_ref + 2e-6 against the fp64 restatement for the
    fp32 normals, the depth and the coefficients; no byte of the uint8 normals more than one level off, at most 1 % differing."""
    checks.check_case(R, "parity")


@pytest.mark.parametrize("name", ["three_cover", "ramp0", "one_wide", "one_high"])
def test_three_tiles_over_a_pixel_ramp_zero_and_images_one_pixel_wide_or_high(R, name):
    checks.check_case(R, name)


def test_a_64_by_64_grid_crosses_the_chunks_of_the_alignment(R):
    """8 x 8 windows at stride 4 on 260 x 260: 4096 tiles, 66 chunks of the alignment"""
    checks.check_case(R, "grid64")


def test_seam_condition_and_planted_case_on_the_device(R):
    checks.check_seam(R)
    checks.check_planted(R)


def test_unaligned_blend_and_raw_views(R):
    checks.check_unaligned_and_raw_views(R)


def test_two_images_in_one_call_equal_two_calls_and_two_runs_are_identical(R):
    checks.check_batch_and_reproducibility(R)


def test_canaries_around_strided_outputs_stay(R):
    checks.check_canaries(R)


def test_non_finite_values_in_one_images_tiles_leave_the_other_image_alone(R):
    checks.check_non_finite(R)


# ------------------------------------------------------------------------------------------------ against the TTA entry points, bit for bit
def test_a_one_by_one_grid_is_the_tta_mean_of_that_one_view():
    size, _, net, _ = CASES["parity"]
    nm, dm, _ = case_maps("parity")
    H, W = size
    n_map, d_map = nm[0].to(DEV).contiguous(), dm[0].to(DEV).contiguous()
    view = [pp.TtaView(0, net[0], net[1], 0, 0, 0, H, W, 0)]
    grid = [pp.TileGrid.make(0, net, size, [0], [0], (24, 37))]                           # both edges on the border: no ramp applies
    for output in ("u8", "f32"):
        for normalize in (True, False):
            want = pp.merge_normal_views_gpu(n_map, view, [size], "mean", normalize, output)[0]
            assert torch.equal(pp.blend_normal_tiles_gpu(n_map, grid, [size], normalize, output)[0], want), (output, normalize)
    want = pp.merge_depth_views_gpu(d_map, view, [size], None, None, "mean", "f32")[0]
    assert torch.equal(pp.blend_depth_tiles_gpu(d_map, grid, [size])[0], want)
    coeffs = torch.tensor([[1.3, -0.1]], device=DEV)
    want = pp.merge_depth_views_gpu(d_map, view, [size], coeffs, None, "mean", "f32")[0]
    assert torch.equal(pp.blend_depth_tiles_gpu(d_map, grid, [size], coeffs)[0], want)


def _tta_coeffs(flat, grid_c, grid, size, tiles):
    """dptx_tta_align_depth's coefficients for the windows of the given tiles (at most 63) and the anchor"""
    H, W = size
    nx, step = grid_c.nx, 4 * grid_c.h * grid_c.w
    views = [pp.TtaView(grid_c.anchor_offset, grid_c.ah, grid_c.aw, 0, 0, 0, H, W, 0)]
    views += [pp.TtaView(grid_c.offset + k * step, grid_c.h, grid_c.w, 0, grid.ys[k // nx], grid.xs[k % nx], grid.ch, grid.cw, 0) for k in tiles]
    return pp.align_depth_views_gpu(flat, views, [0], [size])[0][1:]


def test_tile_coefficients_are_those_of_the_tta_alignment_bit_for_bit():
    for name, tiles in (("parity", range(9)), ("three_cover", range(9)), ("grid64", range(40, 103))):   # 63 tiles across a chunk boundary
        size, grid, _, _ = CASES[name]
        _, dm, anchor = case_maps(name)
        flat, (g,) = pack_tiles([(dm, grid, anchor)])
        flat = flat.to(DEV)
        got = pp.align_depth_tiles_gpu(flat, [g], [size])
        assert got.shape == (len(dm), 2) and bool(torch.isfinite(got).all())
        assert torch.equal(got[tiles.start:tiles.stop], _tta_coeffs(flat, g, grid, size, tiles)), name


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _model(task):
    from omnidata_amd.model import build_model
    return build_model(task, random_weights=0, dtype="bf16", max_batch=8).to(DEV)


def _rgb(h, w, seed):
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


def _tiles_by_hand(model, img, plan, task, with_anchor):
    """-> (flat maps: [anchor |] tiles in grid order, the TileGrid): the forwards in the batches the classes use"""
    buf, descs = pp.pack_images([img])
    dev = buf.to(DEV)
    (ch, cw), parts, off, anchor_offset = plan.window, [], 0, -1
    with torch.no_grad():
        if with_anchor:
            x = pp.views_to_input_gpu(dev, [descs[0]], [False], plan.anchor_net, task)
            parts.append(model(x).reshape(-1))
            anchor_offset, off = 0, parts[0].numel()
        boxes = [(x0, y0, x0 + cw, y0 + ch) for y0 in plan.ys for x0 in plan.xs]
        x = pp.views_to_input_gpu(dev, [pp.window_desc(descs[0], b) for b in boxes], [False] * len(boxes), plan.net, task)
        assert len(boxes) <= 8
        parts.append(model(x).reshape(-1))
    grid = pp.TileGrid.make(4 * off, plan.net, plan.window, plan.ys, plan.xs, plan.ramps, anchor_offset, plan.anchor_net)
    return torch.cat(parts).float().contiguous(), grid


def test_tiled_normals_is_the_pieces_called_by_hand():
    model, img = _model("normal"), _rgb(100, 150, 1)
    plan = tiled.plan_tiles(150, 100, tile=64)
    assert plan.net == (64, 64) and plan.window == (64, 64) and (len(plan.ys), len(plan.xs)) == (2, 3)
    flat, grid = _tiles_by_hand(model, img, plan, "normal", False)
    for output in ("u8", "f32"):
        got = tiled.TiledNormals(model, tile=64, batch_size=8)([img], output=output)
        assert len(got) == 1 and got[0].is_cuda and got[0].shape == ((100, 150, 3) if output == "u8" else (3, 100, 150))
        assert torch.equal(got[0], pp.blend_normal_tiles_gpu(flat, [grid], [(100, 150)], True, output)[0]), output


def test_tiled_depth_is_the_pieces_called_by_hand():
    model, img = _model("depth"), _rgb(100, 150, 2)
    plan = tiled.plan_tiles(150, 100, tile=64)
    flat, grid = _tiles_by_hand(model, img, plan, "depth", True)
    coeffs = pp.align_depth_tiles_gpu(flat, [grid], [(100, 150)])
    for output in ("rgba", "f32"):
        got, got_c = tiled.TiledDepth(model, tile=64, batch_size=8)([img], output=output, return_coeffs=True)
        assert len(got) == 1 and got[0].is_cuda and got[0].shape == ((100, 150, 4) if output == "rgba" else (100, 150))
        assert torch.equal(got[0], pp.blend_depth_tiles_gpu(flat, [grid], [(100, 150)], coeffs, output)[0]), output
        assert len(got_c) == 1 and torch.equal(got_c[0], coeffs)
    flat, grid = _tiles_by_hand(model, img, plan, "depth", False)
    plain, none = tiled.TiledDepth(model, tile=64, align=None, batch_size=8)([img], output="f32", return_coeffs=True)
    assert none == [None] and torch.equal(plain[0], pp.blend_depth_tiles_gpu(flat, [grid], [(100, 150)])[0])


def test_batch_predictor_routes_through_the_tiles_in_input_order_and_excludes_the_other_modes(tmp_path):
    from omnidata_amd.batch_infer import BatchPredictor
    model = _model("normal")
    shapes = [("a", (100, 150)), ("b", (131, 90))]
    (tmp_path / "in").mkdir()
    files = []
    for k, (stem, (h, w)) in enumerate(shapes):
        files.append(str(tmp_path / "in" / f"{stem}.png"))
        _rgb(h, w, 10 + k).save(files[-1])
    bp = BatchPredictor(model, "normal", batch_size=8, tiled=dict(tile=64))
    outs = list(bp.predict(files))
    alone = tiled.TiledNormals(model, tile=64, batch_size=8)
    for f, (stem, (h, w)), o in zip(files, shapes, outs):
        assert o.shape == (h, w, 3) and o.dtype == torch.uint8
        assert torch.equal(o, alone([Image.open(f)])[0]), stem
    bp.predict_to_dir(files[::-1], str(tmp_path / "out"))
    for f, (stem, (h, w)), o in zip(files, shapes, outs):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / f"{stem}_normal.png")), o.cpu().numpy()), stem
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / f"{stem}_rgb.png")), np.asarray(Image.open(f))), stem
    two = tiled.TiledNormals(model, tile=64, batch_size=8, chunk_images=2)([Image.open(f) for f in files])
    assert all(torch.equal(a, b) for a, b in zip(two, outs))                              # an image's result does not depend on its chunk
    for other in (dict(tta="flip"), dict(full_frame="aspect"), dict(full_frame="squash")):
        with pytest.raises(ValueError, match="tiled excludes"):
            BatchPredictor(model, "normal", tiled=True, **other)
    assert BatchPredictor(model, "normal", tiled=None)._runner is None


def test_demo_cli_tiled_depth_writes_files_of_the_images_own_sizes(tmp_path):
    shapes = [("a", (100, 150)), ("b", (140, 96))]
    (tmp_path / "in").mkdir()
    for k, (stem, (h, w)) in enumerate(shapes):
        _rgb(h, w, 20 + k).save(tmp_path / "in" / f"{stem}.png")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo.py"), "--task", "depth", "--img_path", str(tmp_path / "in"),
                        "--output_path", str(out), "--random-weights", "0", "--dtype", "bf16", "--tiled", "--tile_size", "64"],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for stem, (h, w) in shapes:
        depth = Image.open(out / f"{stem}_depth.png")
        assert depth.size == (w, h) and depth.mode == "RGBA" and Image.open(out / f"{stem}_rgb.png").size == (w, h)
