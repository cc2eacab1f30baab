"""csrc/tta.hip compiled for the HOST (tests/tta_cpu_build: a stand-in for the HIP built-ins, blocks and threads run one after
the other) with AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program: the entry point's own launches --
descriptors by value, tile and tap indexing, the selection lists -- against the restatement, with every buffer a heap block of
exactly its size.  No GPU needed; the GPU tests (tests/test_gpu_tta.py) hold the same cases for the device build."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from omnidata_amd import preprocess as pp
from omnidata_amd.tta import plan_views
from tta_restatement import merge_restatement, synthetic_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "tta_cpu_build")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
NORMAL_U8, NORMAL_F32 = 1, 2
BOUND_ABS = 2e-6
SIZE, EDGE = (70, 93), (9, 13)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tta_cpu_build") / "merge"
    r = subprocess.run([CLANG, "-x", "c++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", HERE, "-o", str(exe), os.path.join(HERE, "main.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return str(exe)


def _run(program, tmp_path, maps_per_image, windows_per_image, sizes, mode):
    views, chunks, off = [], [], 0
    for i, (maps, windows) in enumerate(zip(maps_per_image, windows_per_image)):
        for m, (y0, x0, ch, cw, flip) in zip(maps, windows):
            views.append(pp.TtaView(4 * off, m.shape[1], m.shape[2], i, y0, x0, ch, cw, flip))
            chunks.append(m.reshape(-1).numpy())
            off += m.numel()
    u8 = (mode & 15) == NORMAL_U8
    descs, total = pp.output_layout(sizes, "normal_u8" if u8 else "normal_f32")
    files = [str(tmp_path / n) for n in ("maps", "views", "outs", "out")]
    np.concatenate(chunks).astype(np.float32).tofile(files[0])
    open(files[1], "wb").write(bytes((pp.TtaView * len(views))(*views)))
    open(files[2], "wb").write(bytes(descs)[:len(sizes) * C.sizeof(pp.ImageDesc)])
    r = subprocess.run([program, *files[:3], str(mode), str(total), files[3]], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]                       # a sanitizer report ends the program with its text
    raw = np.fromfile(files[3], dtype=np.uint8)
    if u8:
        return [torch.from_numpy(raw[d.offset:d.offset + H * W * 3].reshape(H, W, 3).copy()) for d, (H, W) in zip(descs, sizes)]
    return [torch.from_numpy(raw[d.offset:d.offset + 12 * H * W].copy().view(np.float32).reshape(3, H, W)) for d, (H, W) in zip(descs, sizes)]


@functools.lru_cache(maxsize=None)
def _oasis_case():
    plan = plan_views(SIZE[1], SIZE[0], [(0.8, [192], True), (0.9, [192, 64], True), (1.0, [192, 64, 96, 128, 160], True)])
    windows = [(box[1], box[0], box[3] - box[1], box[2] - box[0], int(flip)) for box, flip, _, _ in plan]
    return tuple(synthetic_view(k, *plan[k][3], windows[k], SIZE) for k in range(40)), tuple(windows)


def _stacked(n):
    windows = [(0, 0, *EDGE, k % 2) for k in range(n)]
    return [synthetic_view(100 + k, 16, 24, windows[k], EDGE, noise=0.2) for k in range(n)], windows


@pytest.mark.parametrize("merger,normalize", [("median", True), ("median", False), ("mean", True)])
def test_host_build_of_the_merge_is_within_the_gpu_tests_bound_and_clean_under_the_sanitizers(program, tmp_path, merger, normalize):
    maps, windows = _oasis_case()
    code = NORMAL_F32 | (pp.TTA_MEAN if merger == "mean" else 0) | (0 if normalize else pp.TTA_RAW_VIEWS)
    r64 = merge_restatement(maps, windows, SIZE, merger, normalize, torch.float64)
    e_ref = float((merge_restatement(maps, windows, SIZE, merger, normalize, torch.float32).double() - r64).abs().max())
    got = _run(program, tmp_path, [maps], [windows], [SIZE], code)[0]
    err = float((got.double() - r64).abs().max())
    print(f"tta host build {merger}{'' if normalize else '+raw'}: e_ref {e_ref:.3e} err {err:.3e}")
    assert err <= 2 * e_ref + BOUND_ABS


def test_host_build_every_class_of_the_selection_two_images_and_the_uint8_addresses(program, tmp_path):
    for n in (1, 2, 8, 9, 17, 33, 64):
        maps, windows = _stacked(n)
        r64 = merge_restatement(maps, windows, EDGE, "median", True, torch.float64)
        e_ref = float((merge_restatement(maps, windows, EDGE, "median", True, torch.float32).double() - r64).abs().max())
        got = _run(program, tmp_path, [maps], [windows], [EDGE], NORMAL_F32)[0]
        assert float((got.double() - r64).abs().max()) <= 2 * e_ref + BOUND_ABS, n
    big, big_w = _oasis_case()
    small, _ = _stacked(2)
    small_w = [(0, 0, 9, 9, 0), (2, 5, 7, 6, 1)]                                  # columns 11-12: no view
    both = _run(program, tmp_path, [small, big], [small_w, big_w], [EDGE, SIZE], NORMAL_F32)
    assert both[0][:, :, 11:].eq(0.5).all()
    assert torch.equal(both[1], _run(program, tmp_path, [big], [big_w], [SIZE], NORMAL_F32)[0])
    # uint8 rows leave through LDS behind a barrier: sequential threads give no meaningful values, the sanitizer checks the addresses
    _run(program, tmp_path, [small, big], [small_w, big_w], [EDGE, SIZE], NORMAL_U8)
