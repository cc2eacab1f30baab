"""3D refocus augmentation, host side (no GPU): the test-side restatement against the reference's goldens, the draw helper
against the reference's recorded draws, the workspace contract of the C ABI, and the build flags of refocus.hip
(tests/test_build_quality.py checks its assembly)."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import refocus_restatement as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "refocus_*.npz")))


def load(path):
    z = np.load(path)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def test_goldens_present():
    names = {os.path.basename(p) for p in GOLDEN}
    assert {"refocus_wide.npz", "refocus_u16_plateau.npz", "refocus_c1_odd.npz", "refocus_zero_min.npz",
            "refocus_seeded.npz"} <= names
    assert sum(os.path.getsize(p) for p in GOLDEN) < 1 << 20


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[8:-4] for p in GOLDEN])
def test_restatement_reproduces_reference(path):
    g = load(path)
    n = int(g["n"])
    q = rs.quantiles(g["depth"], n)
    assert torch.equal(q, g["quantile_vals"])
    out, seg = rs.refocus(g["rgb"], g["depth"], g["focus"], g["aperture"], q)
    assert torch.equal(seg, g["segments"].long())
    d = (out - g["out"].double()).abs().max().item()
    assert d <= 2e-6, d


def test_goldens_cover_the_domain():
    r = {os.path.basename(p)[8:-4]: rs.radii(g["quantile_vals"], g["focus"], g["aperture"])
         for p in GOLDEN for g in [load(p)]}
    shapes = {os.path.basename(p)[8:-4]: tuple(load(p)["rgb"].shape) for p in GOLDEN}
    assert r["wide"].max() * 3 > 2 * shapes["wide"][3]         # a filter wider than twice the image
    assert r["u16_plateau"].max() * 3 > 2 * shapes["u16_plateau"][3]
    assert r["zero_min"].min() < 0                              # q_0 = -eps: a negative radius, no blur
    assert shapes["c1_odd"][1] == 1
    assert (r["wide"] < 0.1).any()                              # the in-focus level is the image itself


def test_draw_helper_reproduces_reference_draws():
    from omnidata_amd.refocus import draw
    g = load(os.path.join(ROOT, "tests", "golden", "refocus_seeded.npz"))
    torch.manual_seed(int(g["seed"]))
    q = rs.quantiles(g["depth"], int(g["n"]))
    idx, ap = draw(g["rgb"].shape[0], int(g["n"]), 0.001, 6, "cpu")
    assert torch.equal(ap, g["aperture"])
    assert torch.equal(torch.gather(q, 1, idx.unsqueeze(1)), g["focus"])
    torch.manual_seed(int(g["seed"]))
    idx2, ap2 = rs.draw(g["rgb"].shape[0], int(g["n"]), 0.001, 6, "cpu")
    assert torch.equal(idx, idx2) and torch.equal(ap, ap2)


def test_cpu_tensors_are_refused():
    from omnidata_amd.refocus import compute_quantiles, refocus_image
    with pytest.raises(ValueError, match="CUDA"):
        compute_quantiles(torch.rand(1, 1, 8, 8), 4)
    with pytest.raises(ValueError, match="CUDA"):
        refocus_image(torch.rand(1, 3, 8, 8), torch.rand(1, 1, 8, 8), 1.0, 1.0, torch.rand(1, 5))


def _ws(B, C, H, W, n):
    from omnidata_amd.engine import load_library
    v = ctypes.c_int64(-1)
    rc = load_library().dptx_refocus_workspace_bytes(B, C, H, W, n, ctypes.byref(v))
    return rc, v.value


def _documented(B, C, H, W, n):
    A = lambda x: (x + 255) // 256 * 256  # noqa: E731
    R, L = 2 * (n + 1), max(H, W)
    return A(B * (66048 + 12 * R)) + A(8 * B * (n + 1) * (L + 4)) + 4 * B * (n + 1) * C * H * W


@pytest.mark.parametrize("shape", [(1, 3, 512, 512, 10), (32, 3, 512, 512, 10), (2, 1, 37, 53, 4), (8, 4, 1, 4097, 32),
                                   (1, 1, 1, 1, 1), (3, 2, 8192, 2048, 2), (1, 3, 2048, 8192, 63)])
def test_workspace_bytes_documented(built_lib, shape):
    rc, v = _ws(*shape)
    assert rc == 0 and v == _documented(*shape)


@pytest.mark.parametrize("shape", [(1, 3, 4097, 4097, 10), (1, 3, 16, 8193, 10), (1, 3, 8193, 16, 10), (1, 0, 8, 8, 10),
                                   (1, 3, 8, 8, 0), (0, 3, 8, 8, 10), (1, 3, 0, 8, 10), (1, 3, 8, 8, -1)])
def test_workspace_bytes_rejects(built_lib, shape):
    from omnidata_amd.engine import load_library
    rc, _ = _ws(*shape)
    assert rc == -1  # DPTX_E_INVALID
    assert load_library().dptx_refocus_workspace_bytes(1, 3, 8, 8, 4, None) == -1


def test_refocus_unit_built_without_packed_fp32():
    from omnidata_amd.build import SOURCE_FLAGS, SOURCES
    assert "refocus.hip" in SOURCES
    assert "-packed-fp32-ops" in SOURCE_FLAGS["refocus.hip"]
