"""csrc/tiles.hip compiled for the HOST (tests/tiled_cpu_build/main.cpp over the stand-in for the HIP built-ins of
tests/tta_cpu_build) with AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program: the entry points' own
launches -- the blends, and the anchor pass, the stats pass and the solve in chunks of 63 tiles -- on the cases and bounds of the
GPU tests (tests/tiled_checks.py), with every buffer a heap block of exactly its size.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from omnidata_amd import preprocess as pp
import tiled_checks as checks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "tiled_cpu_build")
STAND_IN = os.path.join(ROOT, "tests", "tta_cpu_build")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tiled_cpu_build") / "blend_align"
    r = subprocess.run([CLANG, "-x", "c++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", STAND_IN, "-o", str(exe), os.path.join(HERE, "main.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return str(exe)


class HostRunner:
    def __init__(self, program, tmp_path):
        self.program, self.dir = program, tmp_path

    def _run(self, flat, grids, descs, total, task, mode, align):
        files = [str(self.dir / n) for n in ("maps", "grids", "outs", "out", "coeffs")]
        flat.numpy().astype(np.float32).tofile(files[0])
        open(files[1], "wb").write(bytes((pp.TileGrid * len(grids))(*grids)))
        open(files[2], "wb").write(bytes(descs)[:len(grids) * C.sizeof(pp.ImageDesc)])
        r = subprocess.run([self.program, *files[:3], task, str(mode), str(int(align)), str(total), *files[3:]],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()[-3000:]                   # a sanitizer report ends the program with its text
        raw = torch.from_numpy(np.fromfile(files[3], dtype=np.uint8))
        assert raw.numel() == total
        return raw, torch.from_numpy(np.fromfile(files[4], dtype=np.float32).reshape(-1, 2))

    def normals(self, flat, grids, descs, total, mode):
        return self._run(flat, grids, descs, total, "normal", mode, False)[0]

    def depth(self, flat, grids, descs, total, align):
        return self._run(flat, grids, descs, total, "depth", checks.DEPTH_F32, align)


@pytest.fixture
def R(program, tmp_path):
    return HostRunner(program, tmp_path)


@pytest.mark.parametrize("name", ["parity", "three_cover", "ramp0", "one_wide", "one_high", "grid64"])
def test_host_build_is_within_the_gpu_tests_bounds_and_clean_under_the_sanitizers(R, name):
    checks.check_case(R, name)


def test_host_build_seam_planted_unaligned_and_raw_views(R):
    checks.check_seam(R)
    checks.check_planted(R)
    checks.check_unaligned_and_raw_views(R)


def test_host_build_batch_canaries_and_non_finite_values(R):
    checks.check_batch_and_reproducibility(R)
    checks.check_canaries(R)
    checks.check_non_finite(R)
