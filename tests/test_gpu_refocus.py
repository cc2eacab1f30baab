"""3D refocus augmentation on the GPU (omnidata_amd/refocus.py, csrc/refocus.hip) against CPU torch.quantile, the fp64
restatement (tests/refocus_restatement.py) and the reference's goldens (tools/make_refocus_golden.py).  pytest -m gpu."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import refocus_restatement as rs
from gpu_util import smooth
from omnidata_amd import refocus as rf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "refocus_*.npz")))


def depth_case(kind, B, H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind == "random":
        return torch.rand(B, 1, H, W, generator=gen) * 5 + 0.01
    if kind == "ties":
        return torch.randint(0, 7, (B, 1, H, W), generator=gen).float() * 0.25 + 0.5
    if kind == "plateau":  # 16-bit decoded depth with half of the image at the far value 65535
        v = (smooth(gen, B, H, W, 200.0, 9000.0) / 32).round() * 32
        v.view(B, -1)[:, : (H * W) // 2] = 65535.0
        return (v / 65535.0) / torch.tensor(8000.0 / 65535.0)
    if kind == "signed":  # negative values, and zeros of both signs
        d = torch.randn(B, 1, H, W, generator=gen)
        d.view(B, -1)[:, ::7] = 0.0
        d.view(B, -1)[:, 3::11] = -0.0
        return d
    raise ValueError(kind)


@pytest.mark.parametrize("shape", [(2, 512, 512), (3, 37, 53), (1, 1, 4097)])
@pytest.mark.parametrize("kind", ["random", "ties", "plateau", "signed"])
@pytest.mark.parametrize("n", [1, 2, 10, 32])
def test_quantiles_equal_cpu_torch_quantile(shape, kind, n):
    B, H, W = shape
    d = depth_case(kind, B, H, W, seed=B * 131 + H + n)
    got = rf.compute_quantiles(d.cuda(), n).cpu()
    ref = rs.quantiles(d, n)
    assert got.shape == ref.shape == (B, n + 1)
    assert torch.equal(got, ref), (got - ref).abs().max()


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[8:-4] for p in GOLDEN])
def test_reference_goldens(path):
    z = np.load(path)
    g = {k: torch.from_numpy(z[k]) for k in z.files}
    n = int(g["n"])
    q = rf.compute_quantiles(g["depth"].cuda(), n)
    assert torch.equal(q.cpu(), g["quantile_vals"])
    out, seg = rf.refocus_image(g["rgb"].cuda(), g["depth"].cuda(), g["focus"].cuda(), g["aperture"].cuda(), q, return_segments=True)
    assert torch.equal(seg.cpu(), g["segments"].long())
    d = (out.cpu().double() - g["out"].double()).abs().max().item()
    assert d <= 2e-5, d


def focus_aperture(q, mode, gen, L):
    """Per image: focus at quantile 1 (n >= 2) or the midpoint (n = 1); aperture chosen for the coverage `mode`."""
    B, n1 = q.shape
    f = q[:, 1].clone() if n1 > 2 else (q[:, 0] + q[:, 1]) / 2
    rel = (torch.abs(q - f[:, None]) / q).clamp_min(0)
    far = rel.max(1).values.clamp_min(1e-6)
    if mode == "m1":        # the most blurred level at r = 0.2: every level r < 0.1 or M = 1
        ap = 0.2 / far
    elif mode == "wide":    # the most blurred level ~ 6x the longer side: M > 2 max(H, W)
        ap = 6.0 * L / far
    else:                   # log-uniform as the augmentation draws
        ap = torch.exp(torch.rand(B, generator=gen) * (np.log(6) - np.log(1e-3)) + np.log(1e-3)) * 20
    return f.float(), ap.float()


CASES = [  # B, C, H, W, n, depth range, aperture mode
    (1, 3, 48, 64, 10, (0.05, 3.0), "wide"),
    (8, 3, 40, 56, 10, (0.5, 4.0), "draw"),
    (2, 1, 37, 53, 2, (0.3, 2.0), "draw"),
    (3, 4, 33, 70, 32, (0.2, 5.0), "draw"),
    (2, 3, 30, 41, 1, (0.4, 1.6), "draw"),
    (2, 3, 29, 31, 10, (0.2, 3.0), "m1"),
    (1, 3, 1, 300, 10, (0.2, 3.0), "draw"),
    (1, 3, 300, 1, 10, (0.2, 3.0), "wide"),
    (2, 3, 64, 96, 6, (0.0, 1.5), "draw"),   # minimum depth 0: q_0 = -1e-4, a negative radius
    (1, 3, 128, 160, 10, (0.1, 8.0), "wide"),
]


@pytest.mark.parametrize("case", CASES, ids=[f"B{c[0]}C{c[1]}_{c[2]}x{c[3]}_n{c[4]}_{c[6]}" for c in CASES])
def test_refocus_image_vs_fp64_restatement(case):
    B, C, H, W, n, (lo, hi), mode = case
    gen = torch.Generator().manual_seed(B * 1000 + H * 7 + W + n)
    rgb = torch.rand(B, C, H, W, generator=gen)
    depth = smooth(gen, B, H, W, lo, hi)
    q = rf.compute_quantiles(depth.cuda(), n)
    f, ap = focus_aperture(q.cpu(), mode, gen, max(H, W))
    out, seg = rf.refocus_image(rgb.cuda(), depth.cuda(), f.cuda()[:, None], ap.cuda()[:, None], q, return_segments=True)
    ref, rseg = rs.refocus(rgb, depth, f, ap, q.cpu())
    assert torch.equal(seg.cpu(), rseg)
    d = (out.cpu().double() - ref).abs().max().item()
    assert d <= 1e-5, d
    M = [rs.filter_size(r) for r in rs.radii(q.cpu(), f, ap).reshape(-1)]
    if mode == "wide":
        assert max(M) > 2 * max(H, W)
    if mode == "m1":
        assert max(M) == 1 and any(r >= 0.1 for r in rs.radii(q.cpu(), f, ap).reshape(-1))
    if lo == 0.0:
        assert (rs.radii(q.cpu(), f, ap)[:, 0] < 0).all()


def test_seeded_augmentation_matches_restatement_draws_on_cuda():
    gen = torch.Generator().manual_seed(7)
    rgb, depth = torch.rand(4, 3, 64, 80, generator=gen).cuda(), smooth(gen, 4, 64, 80, 0.2, 4.0).cuda()
    torch.manual_seed(99)
    out, seg = rf.RefocusImageAugmentation(10, 0.001, 6, return_segments=True)(rgb, depth)
    torch.manual_seed(99)
    ref, rseg, _, _ = rs.augment(rgb, depth, 10, 0.001, 6)
    assert torch.equal(seg.cpu(), rseg)
    assert (out.cpu().double() - ref).abs().max().item() <= 1e-5


@pytest.mark.parametrize("bad", ["nan", "inf", "-inf"])
def test_nonfinite_depth_raises(bad):
    d = torch.rand(1, 1, 16, 16) + 0.5
    d[0, 0, 3, 4] = float(bad)
    aug = rf.RefocusImageAugmentation(10, 0.001, 6)
    with pytest.raises(ValueError):
        aug(torch.rand(1, 3, 16, 16).cuda(), d.cuda())


def test_zero_quantile_raises():
    d = torch.rand(1, 1, 16, 16) + 0.5
    q = rf.compute_quantiles(d.cuda(), 4)
    q[0, 2] = 0.0  # the reference: int(inf) at :37
    with pytest.raises(ValueError):
        rf.refocus_image(torch.rand(1, 3, 16, 16).cuda(), d.cuda(), q[:, 1:2], torch.ones(1, 1).cuda(), q)


def _write_pair(folder, stem, h, w, rng, grey=False):
    shape = (h, w) if grey else (h, w, 3)
    Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8)).save(os.path.join(folder, f"{stem}_rgb.png"))
    yy, xx = np.mgrid[0:h, 0:w]
    v = (1500 + 6000 * (xx / max(w - 1, 1)) * (0.5 + 0.5 * yy / max(h - 1, 1))).astype(np.uint16)
    Image.fromarray(v).save(os.path.join(folder, f"{stem}_depth_euclidean.png"))


@pytest.mark.parametrize("nq", [None, 4])
def test_demo_refocus_cli(tmp_path, nq):
    rng = np.random.default_rng(3)
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    _write_pair(str(src), "a", 40, 60, rng)
    _write_pair(str(src), "b", 70, 50, rng, grey=True)
    cmd = [sys.executable, os.path.join(ROOT, "demo_refocus.py"), "--input_path", str(src), "--output_path", str(dst), "--seed", "5"]
    if nq:
        cmd += ["--num_quantiles", str(nq)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert sorted(os.listdir(dst)) == ["a_rgb_refocused.png", "b_rgb_refocused.png"]
    sys.path.insert(0, ROOT)
    import demo_refocus as demo
    torch.manual_seed(5)
    n = nq or 10
    for stem, size in (("a", (512, 768)), ("b", (716, 512))):
        got = np.asarray(Image.open(dst / f"{stem}_rgb_refocused.png"))
        assert got.shape == size + (3,)
        rgb, depth = demo.load_rgb(str(src / f"{stem}_rgb.png")), demo.load_depth(str(src / f"{stem}_depth_euclidean.png"))
        ref, _, _, _ = rs.augment(rgb.cuda(), depth.cuda(), n, 0.001, 6.0)
        want = ref[0].mul(255).float().byte().permute(1, 2, 0).numpy()
        assert np.abs(got.astype(int) - want.astype(int)).max() <= 1


def test_refocus_repeat_bitwise():
    gen = torch.Generator().manual_seed(11)
    rgb, depth = torch.rand(3, 3, 96, 128, generator=gen).cuda(), smooth(gen, 3, 96, 128, 0.1, 5.0).cuda()
    outs = []
    for _ in range(2):
        torch.manual_seed(1)
        outs.append(rf.RefocusImageAugmentation(10, 0.001, 6, return_segments=True)(rgb, depth))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(rf.compute_quantiles(depth, 10), rf.compute_quantiles(depth, 10))
