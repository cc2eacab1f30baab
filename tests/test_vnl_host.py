"""Virtual normal loss, host side (no GPU): select_index() against the reference's draws, the restatement against the
reference's goldens (tools/make_vnl_golden.py), its fp64 autograd against the reference's fp32 gradients, the workspace
contract of the C ABI, and the compiled vnl_loss.hip."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

import vnl_restatement as rs
from test_build_quality import disasm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "vnl_*.npz")))
IDS = [os.path.basename(p)[4:-4] for p in GOLDEN]


def load(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def case(g):
    """golden -> first, second [B,H,W] fp32 tensors, the three linear index tensors, fx, fy, delta_z, select"""
    W = g["first"].shape[-1]
    p = rs.linear_indices(g, W)
    return (torch.from_numpy(g["first"][:, 0]), torch.from_numpy(g["second"][:, 0]), p, float(g["fx"]), float(g["fy"]),
            float(g["delta_z"]), bool(g["select"]))


def test_goldens_present_and_small():
    names = {os.path.basename(p) for p in GOLDEN}
    assert {"vnl_unit.npz", "vnl_metric_odd.npz", "vnl_pred_first.npz", "vnl_zeros.npz", "vnl_noselect.npz", "vnl_same.npz",
            "vnl_none.npz"} <= names
    assert all(os.path.getsize(p) < 256 << 10 for p in GOLDEN)
    assert sum(os.path.getsize(p) for p in GOLDEN) < 1 << 20


def test_goldens_cover_the_cases():
    g = {os.path.basename(p)[4:-4]: load(p) for p in GOLDEN}
    assert g["unit"]["first"].shape == (3, 1, 48, 64) and float(g["unit"]["fx"]) == 1.0 and g["unit"]["first"].max() <= 1.0
    assert g["metric_odd"]["first"].shape == (3, 1, 37, 53) and float(g["metric_odd"]["fx"]) > 10 and g["metric_odd"]["first"].max() > 2
    assert np.abs(g["pred_first"]["grad_first"]).max() > 0
    z = g["zeros"]
    assert (z["second"] == 0).mean() > 0.02 and (z["first"] <= float(z["delta_z"])).mean() > 0.02
    assert not bool(g["noselect"]["select"]) and all(bool(g[k]["select"]) for k in g if k != "noselect")
    assert np.array_equal(g["same"]["first"], g["same"]["second"]) and float(g["same"]["loss"]) == 0 and int(g["same"]["K"]) > 0
    assert int(g["none"]["K"]) == 0 and np.isnan(g["none"]["loss"])
    assert sum(int(v["K"]) > 0 for v in g.values()) >= 2


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_select_index_draws_what_the_reference_draws(path):
    from omnidata_amd.virtual_normal_loss import VNL_Loss
    g = load(path)
    H, W = g["first"].shape[-2:]
    mod = VNL_Loss(float(g["fx"]), float(g["fy"]), (H, W), delta_z=float(g["delta_z"]))
    np.random.seed(int(g["seed"]))
    p123 = mod.select_index()
    after = np.random.random()
    assert sorted(p123) == ["p1_x", "p1_y", "p2_x", "p2_y", "p3_x", "p3_y"]
    for k, v in p123.items():
        assert isinstance(v, np.ndarray) and v.shape == (int(H * W * 0.15),) and np.array_equal(v, g[k]), k
    assert after == float(g["after"])   # the generator advanced exactly as under the reference's call


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_restatement_reproduces_reference(path):
    """Mask and K exactly (no golden has a borderline triple: the tool asserts the cap, the goldens as written have none);
    the compacted point groups exactly (one product and one quotient per coordinate); the loss within 1e-5 relative (the
    reference sums in fp32, the restatement in fp64)."""
    g = load(path)
    first, second, p, fx, fy, dz, select = case(g)
    out = rs.forward(first, second, p, fx, fy, dz, select)
    assert int(out["borderline"].sum()) <= 0.001 * out["keep"].numel()
    ok = ~out["borderline"]
    assert torch.equal(out["keep"][ok], torch.from_numpy(g["mask"])[ok])
    if not out["borderline"].any():
        assert out["K"] == int(g["K"])
        P, Q = rs._points(first, p, fx, fy), rs._points(second, p, fx, fy)
        gp = torch.stack([torch.stack(r, -1) for r in P], -2)[out["keep"]]     # [K, 3 (xyz), 3 (point)]
        assert torch.equal(gp, torch.from_numpy(g["groups_first"]))
        ow = out["overwritten"]
        Q = [[torch.where(ow[..., c], torch.tensor(rs.ZERO_FILL), Q[c][j]) for j in range(3)] for c in range(3)]
        gq = torch.stack([torch.stack(r, -1) for r in Q], -2)[out["keep"]]
        assert torch.equal(gq, torch.from_numpy(g["groups_second"]))
    want = float(g["loss"])
    got = float(out["value"])
    assert (np.isnan(want) and np.isnan(got)) or abs(got - want) <= 1e-5 * abs(want), (got, want)


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_restatement_fp64_gradient_agrees_with_reference(path):
    """fp64 autograd of plain_loss against the reference's fp32 autograd, both arguments, outside the kink pixels (at most
    1 % of the pixels with a gradient): the error is the reference's fp32 evaluation, which the tool recorded as e_ref; it
    is reproduced here, and stays under 1e-4 (fp32 rounding, 6e-8, through the cancellation in the cross products of the
    goldens' smooth depths; the second argument is not filtered for collinearity)."""
    g = load(path)
    first, second, p, fx, fy, dz, select = case(g)
    out = rs.forward(first, second, p, fx, fy, dz, select)
    g64 = rs.fp64_gradients(first, second, p, fx, fy, out)
    kink = rs.kink_pixels(p, out, first.shape)
    for name, ref, got in (("first", g["grad_first"][:, 0], g64[0]), ("second", g["grad_second"][:, 0], g64[1])):
        if int(g["K"]) == 0:
            assert not got.any()
            continue
        nz = got != 0
        assert int((kink & nz).sum()) <= 0.01 * int(nz.sum())
        gmax = got.abs().max().item()
        e = (torch.from_numpy(ref).double() - got)[~kink].abs().max().item() / gmax if gmax > 0 else 0.0
        rec = float(g[f"e_ref_{name}"])
        print(f"{name}: e_ref recorded {rec:.3e}, recomputed {e:.3e}, max|g| {gmax:.3e}")
        assert abs(e - rec) <= 1e-3 * rec + 1e-12 and e <= 1e-4


def test_stable_tie_rule_of_the_restatement():
    """Two identical images: every kept loss is tied between them, and the cut drops the copy in the EARLIER image first."""
    g = load(os.path.join(ROOT, "tests", "golden", "vnl_unit.npz"))
    first, second, p, fx, fy, dz, _ = case(g)
    a, b = first[:1].repeat(2, 1, 1), second[:1].repeat(2, 1, 1)
    out = rs.forward(a, b, p, fx, fy, dz, True)
    one = rs.forward(a[:1], b[:1], p, fx, fy, dz, True)
    assert out["K"] == 2 * one["K"] and out["rank"] == out["K"] // 4
    dropped = out["keep"] & ~out["active"]
    assert int(dropped.sum()) == out["rank"]
    assert not (dropped[1] & ~dropped[0]).any()    # a triple dropped in image 1 is dropped in image 0 too
    assert (out["loss"][dropped] <= out["cut"]).all() and (out["loss"][out["active"]] >= out["cut"]).all()


def test_cpu_tensors_and_wrong_sizes_are_refused():
    from omnidata_amd.virtual_normal_loss import VNL_Loss
    x = torch.rand(1, 1, 8, 8)
    with pytest.raises(ValueError, match="CUDA"):
        VNL_Loss(1.0, 1.0, (8, 8))(x, x)


def _ws(B, H, W, n):
    from omnidata_amd.engine import load_library
    v = ctypes.c_int64(-1)
    rc = load_library().dptx_vnl_workspace_bytes(B, H, W, n, ctypes.byref(v))
    return rc, v.value


def _documented(B, H, W, n):
    A = lambda x: (x + 255) // 256 * 256  # noqa: E731
    nblk = min((B * n + 1023) // 1024, 1024)
    snb = min((3 * n + 1023) // 1024, 512)
    return 2 * A(12 * n) + A(1024 * snb) + 4352 + A(40) + A(4 * nblk) + A(8 * nblk) + A(4 * B * n) + A(B * n)


@pytest.mark.parametrize("shape", [(1, 384, 384, 22118), (32, 384, 384, 22118), (3, 37, 53, 294), (1, 1, 4097, 1), (1, 1, 1, 1),
                                   (2, 8192, 2048, 2516582), (7, 2048, 8192, 5), (3, 16, 16, 1 << 29)])
def test_workspace_bytes_documented(built_lib, shape):
    rc, v = _ws(*shape)
    assert rc == 0 and v == _documented(*shape)


@pytest.mark.parametrize("shape", [(1, 4097, 4097, 8), (1, 16, 8193, 8), (1, 8193, 16, 8), (0, 8, 8, 8), (1, 0, 8, 8), (1, 8, 0, 8),
                                   (1, 8, 8, 0), (1, 8, 8, -3), (-1, 8, 8, 8), (1, 8, 8, (1 << 29) + 1), (8, 8, 8, 1 << 28)])
def test_workspace_bytes_rejects(built_lib, shape):
    from omnidata_amd.engine import load_library
    rc, _ = _ws(*shape)
    assert rc == -1  # DPTX_E_INVALID
    assert load_library().dptx_vnl_workspace_bytes(1, 8, 8, 8, None) == -1


def test_vnl_unit_built_with_the_flags_of_the_midas_unit():
    from omnidata_amd.build import SOURCE_FLAGS, SOURCES
    assert "vnl_loss.hip" in SOURCES
    assert SOURCE_FLAGS["vnl_loss.hip"] == SOURCE_FLAGS["midas_loss.hip"] and "-packed-fp32-ops" in SOURCE_FLAGS["vnl_loss.hip"]
    src = open(os.path.join(ROOT, "omnidata_amd", "csrc", "vnl_loss.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    # the shared header must not carry the pragma into refocus.hip, which keeps the compiler's default outside its *_rn helpers
    hdr = open(os.path.join(ROOT, "omnidata_amd", "csrc", "select.h")).read()
    assert '#include "select.h"' in src and not re.search(r"^\s*#\s*pragma\s+clang\s+fp", hdr, flags=re.M)


def test_vnl_no_float_atomics(tmp_path):
    s = disasm("vnl_loss.hip", tmp_path)
    assert not re.search(r"\b(global|flat|buffer|ds)_atomic_\w*(add|pk_add)_f(32|64)\b", s)
    assert re.search(r"\b(global|flat)_atomic_add(_u32)?\b", s)   # the counts and histograms are integer atomics


def test_entry_points_do_not_allocate_or_synchronise():
    src = "".join(open(os.path.join(ROOT, "omnidata_amd", "csrc", f)).read() for f in ("vnl_loss.hip", "select.h"))
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("hipMalloc", "hipFree", "hipMemcpy", "Synchronize", "hipEventQuery", "hipStreamQuery"):
        assert word not in code, word
