"""csrc/tta_depth.hip compiled for the HOST (tests/tta_depth_cpu_build/main.cpp over the stand-in for the HIP built-ins of
tests/tta_cpu_build) with AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program: the entry points' own
launches -- the anchor pass, the stats pass with its records, the solve and the merge -- against the restatement
(tests/tta_depth_restatement.py), with every buffer a heap block of exactly its size.  No GPU needed; the GPU tests
(tests/test_gpu_tta_depth.py) hold the same cases and bounds for the device build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from omnidata_amd import preprocess as pp
from tta_depth_restatement import (EDGE, SIZE, oasis_depth_case, oasis_depth_reference, stacked_depth_case,
                                   stacked_depth_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "tta_depth_cpu_build")
STAND_IN = os.path.join(ROOT, "tests", "tta_cpu_build")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
DEPTH_F32 = 3
BOUND_ABS = 2e-6


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tta_depth_cpu_build") / "align_merge"
    r = subprocess.run([CLANG, "-x", "c++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", STAND_IN, "-o", str(exe), os.path.join(HERE, "main.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return str(exe)


def _run(program, tmp_path, maps_per_image, windows_per_image, anchors, sizes, mode, align=True):
    """-> ([out [H,W] fp32 per image], coeffs [n_views, 2] fp32)"""
    views, chunks, off, first, anc = [], [], 0, 0, []
    for i, (maps, windows, anchor) in enumerate(zip(maps_per_image, windows_per_image, anchors)):
        anc.append(first + anchor)
        first += len(maps)
        for m, (y0, x0, ch, cw, flip) in zip(maps, windows):
            views.append(pp.TtaView(4 * off, m.shape[0], m.shape[1], i, y0, x0, ch, cw, flip))
            chunks.append(m.reshape(-1).numpy())
            off += m.numel()
    descs, total = pp.output_layout(sizes, "depth_f32")
    files = [str(tmp_path / n) for n in ("maps", "views", "outs", "anchors", "out", "coeffs")]
    np.concatenate(chunks).astype(np.float32).tofile(files[0])
    open(files[1], "wb").write(bytes((pp.TtaView * len(views))(*views)))
    open(files[2], "wb").write(bytes(descs)[:len(sizes) * C.sizeof(pp.ImageDesc)])
    np.asarray(anc, dtype=np.int32).tofile(files[3])
    r = subprocess.run([program, *files[:4], str(mode), str(int(align)), str(total), files[4], files[5]],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]                       # a sanitizer report ends the program with its text
    raw = np.fromfile(files[4], dtype=np.uint8)
    outs = [torch.from_numpy(raw[d.offset:d.offset + 4 * H * W].copy().view(np.float32).reshape(H, W)) for d, (H, W) in zip(descs, sizes)]
    return outs, torch.from_numpy(np.fromfile(files[5], dtype=np.float32).reshape(-1, 2))


@pytest.mark.parametrize("merger", ["median", "mean"])
def test_host_build_of_align_and_merge_is_within_the_gpu_tests_bounds_and_clean_under_the_sanitizers(program, tmp_path, merger):
    maps, windows, anchor = oasis_depth_case()
    r64, c64, e_ref, e_ref_c, _ = oasis_depth_reference(merger)
    outs, coeffs = _run(program, tmp_path, [maps], [windows], [anchor], [SIZE], DEPTH_F32 | (pp.TTA_MEAN if merger == "mean" else 0))
    err, err_c = float((outs[0].double() - r64).abs().max()), float((coeffs.double() - c64).abs().max())
    print(f"tta depth host build {merger}: e_ref {e_ref:.3e} err {err:.3e}; e_ref_c {e_ref_c:.3e} err_c {err_c:.3e}")
    assert coeffs[anchor].tolist() == [1.0, 0.0]
    assert err_c <= 2 * e_ref_c + BOUND_ABS
    assert err <= 2 * e_ref + BOUND_ABS


def test_host_build_every_class_of_the_selection_and_two_images_in_one_call(program, tmp_path):
    for n in (1, 2, 3, 8, 9, 16, 17, 32, 33, 63, 64):
        maps, windows, anchor = stacked_depth_case(n)
        r64, c64, e_ref, e_ref_c = stacked_depth_reference(n, "median")
        outs, coeffs = _run(program, tmp_path, [maps], [windows], [anchor], [EDGE], DEPTH_F32)
        assert float((coeffs.double() - c64).abs().max()) <= 2 * e_ref_c + BOUND_ABS, n
        assert float((outs[0].double() - r64).abs().max()) <= 2 * e_ref + BOUND_ABS, n
    big, big_w, big_a = oasis_depth_case()
    small, small_w, small_a = stacked_depth_case(9)
    both, coeffs = _run(program, tmp_path, [small, big], [small_w, big_w], [small_a, big_a], [EDGE, SIZE], DEPTH_F32)
    alone, coeffs_alone = _run(program, tmp_path, [big], [big_w], [big_a], [SIZE], DEPTH_F32)
    assert torch.equal(both[1], alone[0]) and torch.equal(coeffs[9:], coeffs_alone)
    # coeffs == NULL: the unaligned merge needs neither anchors nor a workspace
    r64, _, e_ref, _, _ = oasis_depth_reference("median", align=False)
    plain, _ = _run(program, tmp_path, [big], [big_w], [big_a], [SIZE], DEPTH_F32, align=False)
    assert float((plain[0].double() - r64).abs().max()) <= 2 * e_ref + BOUND_ABS
