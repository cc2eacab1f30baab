"""MiDaS loss, host side (no GPU): the restatement against the reference's goldens, its closed-form gradient against
autograd of the plain fp64 formulation, the workspace contract of the C ABI, and the compiled midas_loss.hip."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

import midas_restatement as rs
from test_build_quality import disasm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "midas_*.npz")))
LOSS_GOLDEN = [p for p in GOLDEN if not p.endswith("_parts.npz")]


def load(path):
    z = np.load(path)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def test_goldens_present_and_small():
    names = {os.path.basename(p) for p in GOLDEN}
    assert {"midas_smooth.npz", "midas_batch_s3.npz", "midas_masks.npz", "midas_ties.npz", "midas_odd.npz",
            "midas_parts.npz"} <= names
    assert all(os.path.getsize(p) < 256 << 10 for p in GOLDEN)
    assert sum(os.path.getsize(p) for p in GOLDEN) < 1 << 20


def rel_close(a, b, rel):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    both_nan = torch.isnan(a) & torch.isnan(b)
    return bool((both_nan | ((a - b).abs() <= rel * b.abs())).all())


@pytest.mark.parametrize("path", LOSS_GOLDEN, ids=[os.path.basename(p)[6:-4] for p in LOSS_GOLDEN])
def test_restatement_reproduces_reference(path):
    """The reference computes in fp32 (sums included), the restatement sums in fp64: losses within 1e-5 relative (fp32 sums
    of ~1e4 terms drift by a few 1e-7), gradients within 1e-4 max|g| outside the L1 kinks and the median's tie set."""
    g = load(path)
    out = rs.forward(g["pred"][:, 0], g["target"][:, 0], g["mask"][:, 0], rs.ALL, int(g["scales"]), bool(g["image_based"]),
                     float(g["alpha"]), grad_losses=(1.0, 0.0, 0.0))
    assert rel_close(out["losses"], g["losses"], 1e-5), (out["losses"], g["losses"])
    rs.assert_grad_matches_reference(out["grad"], g["grad"][:, 0], g["pred"][:, 0], g["mask"][:, 0], out)


def test_restatement_reproduces_reference_parts():
    g = load(os.path.join(ROOT, "tests", "golden", "midas_parts.npz"))
    p, t, m = g["pred"][:, 0], g["target"][:, 0], g["mask"][:, 0]
    o = rs.forward(p, t, m, rs.SSI)
    assert rel_close(o["ssi"], g["ssi"], 1e-5)
    for got, ref in ((o["pred_aligned"], g["pred_aligned"][:, 0]), (o["target_aligned"], g["target_aligned"][:, 0])):
        assert (got.double() - ref.double()).abs().max() <= 1e-5 * ref.abs().max()
    o = rs.forward(p, t, m, rs.GRAD | rs.ALIGN)
    # the reference sums in fp32 (worst case n 2^-24 relative) and the 2x2 solve amplifies that by kappa = a00 a11 / det
    md, pd = m.double(), p.double()
    a00, a01, n = (md * pd * pd).sum((1, 2)), (md * pd).sum((1, 2)), md.sum((1, 2))
    bound = n * 2.0 ** -24 * a00 * n / (a00 * n - a01 * a01)
    for k in ("scale", "shift"):
        assert ((o[k].double() - g[k].double()).abs() <= bound * g[k].double().abs()).all(), (k, o[k], g[k], bound)
    assert rel_close(rs.forward(p, t, m, rs.GRAD, 4, False)["reg"], g["gm_batch_s4"], 1e-5)
    assert rel_close(rs.forward(p, t, m, rs.GRAD, 3, True)["reg"], g["gm_image_s3"], 1e-5)


def test_goldens_cover_the_edge_cases():
    g = load(os.path.join(ROOT, "tests", "golden", "midas_masks.npz"))
    n = g["mask"].reshape(g["mask"].shape[0], -1).sum(1)
    assert n[1] == 0 and n[2] == 1 and 0 < n[3] < 0.02 * g["mask"][0].numel()
    g = load(os.path.join(ROOT, "tests", "golden", "midas_ties.npz"))
    p, m = g["pred"][:, 0], g["mask"][:, 0]
    t, _ = rs.medians(p.reshape(p.shape[0], -1), m.reshape(p.shape[0], -1))
    assert all(int((m[b] & (p[b] == t[b])).sum()) > 10 for b in range(p.shape[0]))
    assert not bool(load(os.path.join(ROOT, "tests", "golden", "midas_batch_s3.npz"))["image_based"])


CLOSED_FORM = [  # terms, scales, image_based, alpha, B, H, W
    (rs.ALL, 4, True, 0.1, 3, 20, 24),
    (rs.ALL, 3, False, 0.5, 2, 17, 23),
    (rs.SSI, 1, True, 0.1, 3, 16, 16),
    (rs.GRAD, 4, False, 0.1, 2, 19, 21),
    (rs.GRAD, 2, True, 0.1, 2, 19, 21),
    (rs.GRAD | rs.ALIGN, 3, True, 0.1, 2, 18, 20),
]


@pytest.mark.parametrize("case", CLOSED_FORM, ids=[f"t{c[0]}_s{c[1]}_{'img' if c[2] else 'batch'}" for c in CLOSED_FORM])
def test_closed_form_gradient_equals_fp64_autograd(case):
    """Well-conditioned fp64 data (continuous values: no ties, no kinks): the closed form of the restatement equals
    autograd of the plain formulation, losses and gradient, within 1e-10 relative."""
    terms, scales, image_based, alpha, B, H, W = case
    gen = torch.Generator().manual_seed(B * 100 + H + W + terms)
    t = torch.rand(B, H, W, generator=gen, dtype=torch.float64) * 4 + 0.5
    p = (0.6 * t + 0.4 + 0.3 * torch.rand(B, H, W, generator=gen, dtype=torch.float64)).requires_grad_(True)
    m = torch.rand(B, H, W, generator=gen) < 0.8
    gl = (1.0, 0.25, 0.5)
    out = rs.forward(p.detach(), t, m, terms, scales, image_based, alpha, dt=torch.float64, grad_losses=gl)
    alpha32 = float(np.float32(alpha))
    total, ssi, reg = rs.plain_loss(p, t, m, terms, scales, image_based, alpha32)
    (gl[0] * total + gl[1] * ssi + gl[2] * reg).backward()
    want = torch.stack([total.detach(), ssi.detach(), torch.as_tensor(reg).detach()]).double()
    assert ((out["losses"] - want).abs() <= 1e-10 * want.abs().max()).all(), (out["losses"], want)
    d = (out["grad"] - p.grad).abs().max().item()
    assert d <= 1e-10 * p.grad.abs().max().item(), d


def test_cpu_tensors_are_refused():
    from omnidata_amd.midas_loss import MidasLoss, compute_scale_and_shift
    x = torch.rand(1, 1, 8, 8)
    with pytest.raises(ValueError, match="CUDA"):
        MidasLoss()(x, x, x > 0.5)
    with pytest.raises(ValueError, match="CUDA"):
        compute_scale_and_shift(x[:, 0], x[:, 0], x[:, 0] > 0.5)


def _ws(B, H, W, scales):
    from omnidata_amd.engine import load_library
    v = ctypes.c_int64(-1)
    rc = load_library().dptx_midas_workspace_bytes(B, H, W, scales, ctypes.byref(v))
    return rc, v.value


def _documented(B, H, W):
    A = lambda x: (x + 255) // 256 * 256  # noqa: E731
    nblk = min((H * W + 4095) // 4096, 1024)
    return A(256 + 8256 * B) + A(80 * B) + A(256 * B) + A(128 * B) + A(128 * B * nblk)


@pytest.mark.parametrize("shape", [(8, 384, 384, 4), (32, 384, 384, 4), (3, 37, 53, 1), (1, 1, 4097, 8), (1, 1, 1, 1),
                                   (2, 8192, 2048, 4), (7, 2048, 8192, 3)])
def test_workspace_bytes_documented(built_lib, shape):
    rc, v = _ws(*shape)
    assert rc == 0 and v == _documented(*shape[:3])


@pytest.mark.parametrize("shape", [(1, 4097, 4097, 4), (1, 16, 8193, 4), (1, 8193, 16, 4), (0, 8, 8, 4), (1, 0, 8, 4),
                                   (1, 8, 0, 4), (1, 8, 8, 0), (1, 8, 8, 9), (-1, 8, 8, 4)])
def test_workspace_bytes_rejects(built_lib, shape):
    from omnidata_amd.engine import load_library
    rc, _ = _ws(*shape)
    assert rc == -1  # DPTX_E_INVALID
    assert load_library().dptx_midas_workspace_bytes(1, 8, 8, 4, None) == -1


def test_midas_unit_built_without_packed_fp32():
    from omnidata_amd.build import SOURCE_FLAGS, SOURCES
    assert "midas_loss.hip" in SOURCES
    assert "-packed-fp32-ops" in SOURCE_FLAGS["midas_loss.hip"]


def test_midas_no_float_atomics(tmp_path):
    s = disasm("midas_loss.hip", tmp_path)
    assert not re.search(r"\b(global|flat|buffer|ds)_atomic_\w*(add|pk_add)_f(32|64)\b", s)


def test_entry_points_do_not_allocate_or_synchronise():
    src = "".join(open(os.path.join(ROOT, "omnidata_amd", "csrc", f)).read() for f in ("midas_loss.hip", "select.h"))
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("hipMalloc", "hipFree", "hipMemcpy", "Synchronize", "hipEventQuery", "hipStreamQuery"):
        assert word not in code, word
