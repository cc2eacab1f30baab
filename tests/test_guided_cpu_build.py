"""csrc/guided.hip compiled for the HOST (tests/guided_cpu_build/main.cpp over the stand-in header of tests/tta_cpu_build: blocks and
threads run one after the other) with AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program: the entry point's
own launches -- descriptors by value, tile and footprint geometry, tap addresses in LDS and in memory, guide reads with padded
rows, the uint8 rows -- on the small shapes of tests/guided_cases.py, with every buffer a heap block of exactly its size.

The kernel exchanges data through LDS (the staged footprint, the uint8 rows, the min / max reduction), and the stand-in runs the
threads one after another.  main.cpp runs every block three times, which makes the staged footprint exact in the second run and
the uint8 rows in the third, so the three modes without a reduction are also compared with the restatement here; for DEPTH_RGBA only the addresses
are checked on the host, the values are checked on the GPU (tests/test_gpu_guided.py).  Nothing here loads sanitized code into
Python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from omnidata_amd import preprocess as pp
from guided_cases import CALLS, RADII, SIGMA_SPACE, inputs, pack_guides, restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "guided_cpu_build")
STANDIN = os.path.join(ROOT, "tests", "tta_cpu_build")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
RENORM = pp.RESIZE_RENORM
SIGMA_RANGE = 0.25


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("guided_cpu_build") / "guided"
    r = subprocess.run([CLANG, "-x", "c++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", STANDIN, "-o", str(exe), os.path.join(HERE, "main.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return str(exe)


def _run(program, tmp_path, name, mode, renormalize, radius):
    h, w, sizes = CALLS[name][:3]
    Cn = 3 if mode.startswith("normal") else 1
    S, G_lo, guides = inputs(name, Cn)
    pixels, gdescs = pack_guides(name, guides)
    outs, total = pp.output_layout(sizes, mode)
    files = [str(tmp_path / n) for n in ("y", "lo", "pixels", "guides", "outs", "out")]
    S.numpy().tofile(files[0])
    G_lo.numpy().tofile(files[1])
    pixels.tofile(files[2])
    open(files[3], "wb").write(bytes((pp.ImageDesc * len(gdescs))(*[pp.ImageDesc(*d) for d in gdescs])))
    open(files[4], "wb").write(bytes(outs)[:len(sizes) * C.sizeof(pp.ImageDesc)])
    code = pp.RESIZE_MODES[mode] | (RENORM if renormalize else 0)
    r = subprocess.run([program, *files[:5], str(Cn), str(h), str(w), str(code), str(radius), str(SIGMA_SPACE), str(SIGMA_RANGE),
                        str(total), files[5]], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]                       # a sanitizer report ends the program with its text
    raw = torch.from_numpy(np.fromfile(files[5], dtype=np.uint8))
    return pp._output_views(raw, outs, sizes, mode)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_host_build_is_clean_under_the_sanitizers_and_within_the_gpu_tests_bound(program, tmp_path, name):
    for radius in RADII:
        for mode, renorm in (("normal_f32", False), ("normal_f32", True), ("depth_f32", False)):
            r64 = restated(name, mode, renorm, radius, SIGMA_RANGE, torch.float64)
            r32 = restated(name, mode, renorm, radius, SIGMA_RANGE, torch.float32)
            E = max(float((a.double() - b).abs().max()) for a, b in zip(r32, r64))
            got = _run(program, tmp_path, name, mode, renorm, radius)
            err = max(float((a.double() - b).abs().max()) for a, b in zip(got, r64))
            print(f"guided host build {name} R={radius} {mode}{'+renorm' if renorm else ''}: E {E:.3e} err {err:.3e} ratio {err / E:.2f}")
            assert err <= 4 * E
        r64 = restated(name, "normal_u8", True, radius, SIGMA_RANGE, torch.float64)
        got = _run(program, tmp_path, name, "normal_u8", True, radius)
        diff = torch.cat([(a.int() - b.int()).abs().reshape(-1) for a, b in zip(got, r64)])
        assert int(diff.max()) <= 1 and int((diff > 0).sum()) <= 0.001 * diff.numel()
        _run(program, tmp_path, name, "depth_rgba", False, radius)          # addresses only: the reduction goes through LDS
