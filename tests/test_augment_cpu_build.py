"""csrc/augment.hip compiled for the HOST (tests/augment_cpu_build/main.cpp over the stand-in header of tests/tta_cpu_build) with
AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program: the entry points' own launches -- tile and halo
geometry, the LDS regions of the three stages, the reflected taps, the gather's descriptors by value -- on the shapes of the GPU
tests (tests/augment_cases.py), with every buffer a heap block of exactly its size.  main.cpp runs every block four times, which
makes each stage's LDS buffer complete before the stage behind it reads it, so the values are compared with the restatement at
the GPU tests' bar.  No GPU needed; nothing here loads sanitized code into Python."""
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_cases as cases
import augment_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "augment_cpu_build")
STANDIN = os.path.join(ROOT, "tests", "tta_cpu_build")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("augment_cpu_build") / "augment"
    r = subprocess.run([CLANG, "-x", "c++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", STANDIN, "-o", str(exe), os.path.join(HERE, "main.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return str(exe)


def _run(args):
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]           # a sanitizer report ends the program with its text
    return int(r.stdout.decode().strip())


def run_chain(program, tmp_path, x, plan):
    files = {}
    for name, a in (("x", x.numpy()), ("sharp", plan.sharp), ("motion", plan.motion), ("gy", plan.gy), ("gx", plan.gx)):
        if a is None:
            files[name] = "-"
        else:
            files[name] = str(tmp_path / name)
            np.ascontiguousarray(a, dtype=np.float32).tofile(files[name])
    out = str(tmp_path / "out")
    km = 0 if plan.motion is None else plan.motion.shape[-1]
    kgy, kgx = (0, 0) if plan.gy is None else (plan.gy.shape[-1], plan.gx.shape[-1])
    rc = _run([program, "chain", files["x"], *map(str, x.shape), files["sharp"], files["motion"], str(km), files["gy"], files["gx"],
               str(kgy), str(kgx), out])
    return rc, torch.from_numpy(np.fromfile(out, dtype=np.float32)).view(x.shape)


# the host build runs every block four times under the sanitizers: half of the GPU tests' cases, every shape and combination among them
HOST_CASES = cases.cases()[::2]


@pytest.mark.parametrize("case", HOST_CASES, ids=cases.case_id)
def test_chain_host_build_is_clean_under_the_sanitizers_and_within_the_gpu_tests_bar(program, tmp_path, case):
    H, W, C = case[:3]
    x = cases.image(C, H, W)
    plan = cases.plan_of(case)
    rc, got = run_chain(program, tmp_path, x, plan)
    assert rc == 0
    cases.judge(got, x, plan, "host build " + cases.case_id(case))


def test_chain_host_build_rejects_what_the_header_rejects(program, tmp_path):
    x = cases.image(1, 3, 9)
    import omnidata_amd.augmentation as A
    assert run_chain(program, tmp_path, x, A.plan_filter_chain(3, gaussian=((7, 3), 1.0)))[0] == -1     # H = 3 <= 7 // 2
    assert run_chain(program, tmp_path, x, A.ChainPlan(3))[0] == -1                                       # no stage


def run_resize(program, tmp_path, tensors, interps, op, y0, x0, h, w):
    B, _, Hs, Ws = tensors[0].shape
    args, outs = [], []
    for i, (t, interp) in enumerate(zip(tensors, interps)):
        src, out = str(tmp_path / f"src{i}"), str(tmp_path / f"out{i}")
        t.numpy().tofile(src)
        args += [src, str(t.shape[1]), "0" if t.dtype == torch.float32 else "1", str(interp), out]
        outs.append(out)
    rc = _run([program, "resize", *map(str, (B, Hs, Ws, op, y0, x0, h, w, len(tensors))), *args])
    got = [torch.from_numpy(np.fromfile(o, dtype=t.numpy().dtype)).view(B, t.shape[1], h, w) for o, t in zip(outs, tensors)]
    return rc, got


@pytest.mark.parametrize("src,dst", [((72, 80), (48, 48)), ((80, 72), (64, 48)), ((37, 53), (53, 37)), ((20, 130), (17, 65))])
def test_gather_host_build_crop_nearest_bilinear(program, tmp_path, src, dst):
    g = torch.Generator().manual_seed(5)
    rgb = torch.rand(2, 3, *src, generator=g)
    depth = torch.rand(2, 1, *src, generator=g)
    mask = (torch.rand(2, 1, *src, generator=g) < 0.5).to(torch.uint8)
    h, w = dst
    rc, got = run_resize(program, tmp_path, [rgb, depth, mask], [0, 1, 1], 1, 0, 0, h, w)
    assert rc == 0
    assert torch.equal(got[1], F.interpolate(depth, (h, w), mode="nearest")) and torch.equal(got[1], R.resize_nearest(depth, h, w))
    assert torch.equal(got[2], R.resize_nearest(mask, h, w))
    r64, r32 = R.resize_bilinear(rgb, h, w, torch.float64), R.resize_bilinear(rgb, h, w, torch.float32)
    E = float((r32.double() - r64).abs().max())
    assert float((got[0].double() - r64).abs().max()) <= 2 * E + 2e-6
    if h <= src[0] and w <= src[1]:
        y0, x0 = src[0] - h, (src[1] - w) // 2
        rc, got = run_resize(program, tmp_path, [rgb, depth, mask], [0, 1, 1], 0, y0, x0, h, w)
        assert rc == 0
        for a, t in zip(got, (rgb, depth, mask)):
            assert torch.equal(a, R.crop(t, y0, x0, h, w))
        assert run_resize(program, tmp_path, [rgb], [0], 0, y0 + 1, x0, h, w)[0] == -1                    # one row below the source
