"""Surface-normal loss, host side (no GPU): the goldens (tools/make_normal_golden.py) cover their cases, the restatement
(tests/normal_restatement.py) against them, the reference's own fp32 error inside the bounds the GPU tests use, the
workspace contract of the C ABI, and the compiled normal_loss.hip.

Loss bounds (shared with tests/test_gpu_normal.py), u = 2^-24 the unit roundoff of fp32, against values evaluated in fp64:
  l1     every |p - t| is one rounding (relative u) and the sum is exact to fp64; the quotient is rounded once more:
         |l1 - l1_64| <= 2 u l1_64.
  cos    per pixel 16 u.  To first order: x = clamp(2 p - 1) is one rounding of a value in [-1, 1] (u); the three squares and
         their two additions move |x|^2 by at most 3 u relative, the root halves that and rounds (2.5 u), the quotient rounds
         once more, so each component of the unit vector carries at most 4.5 u of a value of at most 1, for prediction and
         target alike; a product of two components carries 4.5 u + 4.5 u + u = 10 u of |xh_c yh_c|, and sum_c |xh_c yh_c| <= 1
         (Cauchy-Schwarz), so the dot product carries 10 u plus 2 u for its two additions of partial sums of at most 1: 12 u.
         That count drops the second-order terms, so it is no proof of a tighter constant: the issue's 16 u stands.  The mean
         of N such values carries no more, and its final rounding one more u: |cos - cos_64| <= 17 u.
  total  the sum with l1_weight from the fp64 values, plus one rounding: 17 u + l1_weight 2 u l1_64 + u |total_64|.
"""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import normal_restatement as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_CASES = ("unit", "odd", "clamp", "degenerate", "empty")
U = 2.0 ** -24


def load(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", f"normal_{name}.npz"))
    return {k: z[k] for k in z.files}


def case(g):
    return (torch.from_numpy(g["pred"]), torch.from_numpy(g["target"]), torch.from_numpy(g["mask"])[:, 0], int(g["flags"]),
            float(g["l1_weight"]))


def loss_bounds(ref64, l1_weight):
    """(total, l1, cos) bounds of the module docstring around the fp64 losses ref64"""
    total, l1, cos = (abs(float(v)) for v in ref64)
    b_l1, b_cos = 2 * U * l1, 17 * U
    return np.array([b_cos + l1_weight * b_l1 + U * total, b_l1, b_cos])


def within(got, ref64, l1_weight):
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    if np.isnan(ref64).any():
        return bool(np.array_equal(np.isnan(got), np.isnan(ref64)))
    return bool((np.abs(got - ref64) <= loss_bounds(ref64, l1_weight)).all())


def test_goldens_present_and_small():
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "normal_*.npz")))
    names = {os.path.basename(p)[7:-4] for p in paths}
    assert set(LOSS_CASES) | {"masked", "validmask"} <= names
    assert all(os.path.getsize(p) < 256 << 10 for p in paths)
    assert sum(os.path.getsize(p) for p in paths) < 1 << 20


def test_goldens_cover_the_cases():
    g = {k: load(k) for k in LOSS_CASES}
    assert g["unit"]["pred"].shape == (2, 3, 32, 48) and 0.0 <= g["unit"]["pred"].min() and g["unit"]["pred"].max() <= 1.0
    assert 0.7 < g["unit"]["mask"].mean() < 0.8
    o = g["odd"]
    assert o["pred"].shape == (2, 3, 37, 53) and o["pred"].min() < 0 and o["pred"].max() > 1 and not int(o["flags"]) & rs.CLAMP_PRED
    c = g["clamp"]
    assert int(c["flags"]) & rs.CLAMP_PRED and c["pred"].min() < 0 and c["pred"].max() > 1
    m3 = np.repeat(c["mask"], 3, 1)
    assert ((c["pred"] == 0) & m3).any() and ((c["pred"] == 1) & m3).any()          # on the ends, where the gradient passes
    assert not c["grad_total"][(c["pred"] < 0) | (c["pred"] > 1)].any() and c["grad_total"][(c["pred"] == 1) & m3].any()
    d = g["degenerate"]
    m = d["mask"][:, 0]
    off = np.abs(d["pred"] - 0.5)
    kinds = dict(zero=(d["pred"] == 0.5).all(1), tiny=((off > 0) & (off < 2e-6)).all(1), same=(d["pred"] == d["target"]).all(1),
                 zero_target=(d["target"] == 0.5).all(1))
    for k, v in kinds.items():
        assert (v & m).sum() >= 1, k
    assert np.abs(d["grad_total"]).max() > 1e8        # the zero vector's gradient, -2 yh / (eps N)
    e = g["empty"]
    assert not e["mask"].any() and np.isnan(e["losses"]).all() and np.isnan(e["losses64"]).all()
    assert not e["grad_total"].any() and not e["grad_cos"].any()
    mk = load("masked")
    assert mk["mask"].shape == (2, 3, 17, 19) and (mk["mask"][:, 0] != mk["mask"][:, 1]).any()
    assert np.isnan(mk["l1_empty"]) and np.isnan(mk["mse_empty"]) and float(mk["value_empty"]) == 0.0
    v = load("validmask")
    shapes = set()
    for i in range(int(v["count"])):
        m, valid = v[f"m{i}"], v[f"valid{i}"]
        shapes.add((m.shape, int(v[f"pool{i}"])))
        assert np.isnan(m).any() and (m > 1).any() and ((m > 0) & (m < 1)).any() and valid.shape == m.shape
        assert (m[:, :, -1, :] == 0).any() and (m[:, :, :, -1] == 0).any()
    assert shapes == {(s, k) for s in ((1, 1, 8, 8), (2, 1, 37, 53), (1, 1, 5, 4)) for k in (4, 3)}


@pytest.mark.parametrize("name", LOSS_CASES)
def test_restatement_reproduces_reference(name):
    """Losses within the derived bounds of the reference's fp64 values (fp32 terms and fp64 terms alike), and the fp64
    autograd within e_ref, by its definition, of the reference's fp32 gradients.  Of the two gradient clauses `e <= 1e-6`
    carries the weight: it bounds the distance between the restatement's fp64 autograd and the reference's fp32 gradients.
    The comparison with the recorded e_ref only pins the file, since tools/make_normal_golden.py computed that number with
    this same restatement."""
    g = load(name)
    pred, target, mask, flags, w = case(g)
    out = rs.evaluate(pred, target, mask, flags, w, (1.0, 0.0, 0.0))
    print(name, "restatement", out["losses32"].tolist(), out["losses64"].tolist(), "reference fp64", g["losses64"].tolist())
    assert within(out["losses32"].numpy(), g["losses64"], w)
    assert within(out["losses64"].numpy(), g["losses64"], w)
    if out["N"] == 0:
        assert not out["grad"].any() and not g["grad_total"].any()
        return
    for key, fl, gl, e_key in (("grad_total", flags, (1.0, 0.0, 0.0), "e_ref"),
                               ("grad_cos", (flags & rs.CLAMP_PRED) | rs.COS, (0.0, 0.0, 1.0), "e_ref_cos")):
        o = rs.evaluate(pred, target, mask, fl, w, gl)
        e = rs.scaled_error(torch.from_numpy(g[key]), o["grad"], rs.gradient_scale(o, fl, w, gl))
        print(f"{name} {key}: e {e:.3e}, recorded {float(g[e_key]):.3e}")
        assert abs(e - float(g[e_key])) <= 1e-6 * e + 1e-15 and e <= 1e-6
        assert not o["grad"][~mask.unsqueeze(1).expand_as(o["grad"])].any()


@pytest.mark.parametrize("name", LOSS_CASES)
def test_reference_fp32_losses_lie_within_the_bounds(name):
    """The bounds are ones the reference alone meets: its fp32 losses against its fp64 losses."""
    g = load(name)
    d = np.abs(g["losses"].astype(np.float64) - g["losses64"])
    print(name, "|fp32 - fp64| of the reference (total, l1, cos):", d.tolist(), "bounds", loss_bounds(g["losses64"], float(g["l1_weight"])).tolist()
          if not np.isnan(d).any() else "NaN")
    assert within(g["losses"], g["losses64"], float(g["l1_weight"]))


def test_restatement_masked_losses_and_valid_mask_reproduce_reference():
    g = load("masked")
    pred, target, mask = (torch.from_numpy(g[k]) for k in ("pred", "target", "mask"))
    N = int(mask.sum())
    for key, kind in (("l1", rs.MASKED_L1), ("mse", rs.MASKED_MSE), ("value", rs.MASKED_VALUE | rs.MASKED_EMPTY_ZERO)):
        l32, l64, grad, n = rs.masked(pred, target, mask, kind, grad=True)
        assert n == N
        # two roundings per element at most (the difference, the square), the fp64 sum exact, one final rounding
        assert abs(float(l32) - float(g[f"{key}_64"])) <= 3 * U * abs(float(g[f"{key}_64"]))
        assert abs(float(l64) - float(g[f"{key}_64"])) <= 1e-12
        assert abs(float(g[key]) - float(g[f"{key}_64"])) <= 1e-5 * abs(float(g[f"{key}_64"]))   # the reference sums in fp32
        ref = torch.from_numpy(g[f"grad_{key}"]).double()
        assert ((ref - grad).abs() <= 4 * U * grad.abs()).all() and torch.equal(ref != 0, grad != 0)
        e32, e64, egrad, n0 = rs.masked(pred, target, torch.zeros_like(mask), kind, grad=True)
        want = float(g[f"{key}_empty"])
        assert n0 == 0 and not egrad.any() and not g[f"grad_{key}_empty"].any()
        assert (np.isnan(want) and torch.isnan(e32) and torch.isnan(e64)) or (want == 0.0 and float(e32) == 0.0 and float(e64) == 0.0)
    v = load("validmask")
    for i in range(int(v["count"])):
        m, pool = torch.from_numpy(v[f"m{i}"]), int(v[f"pool{i}"])
        assert torch.equal(rs.valid_mask(m, pool), torch.from_numpy(v[f"valid{i}"])), i


@pytest.mark.parametrize("pool", [2, 3, 4])
def test_valid_mask_index_formula_is_torch_nearest(pool):
    """the restatement against max_pool2d + F.interpolate(mode='nearest') themselves, on sizes around multiples of the pool"""
    gen = torch.Generator().manual_seed(pool)
    for H, W in ((pool, pool), (pool + 1, 2 * pool - 1), (37, 53), (64, 96), (130, 7), (7, 130)):
        m = (torch.rand(2, 1, H, W, generator=gen) < 0.97).float()
        m[0, 0, H // 2, W // 2] = float("nan")
        pooled = torch.nn.functional.max_pool2d(1 - m, kernel_size=pool)
        want = torch.nn.functional.interpolate(pooled, (H, W), mode="nearest") == 0
        assert torch.equal(rs.valid_mask(m, pool), want), (H, W)


def test_cpu_tensors_are_refused():
    from omnidata_amd import normal_loss as nl
    x = torch.rand(1, 3, 8, 8)
    m = torch.ones(1, 1, 8, 8, dtype=torch.bool)
    with pytest.raises(ValueError, match="CUDA"):
        nl.NormalLoss()(x, x, m)
    with pytest.raises(ValueError, match="CUDA"):
        nl.masked_l1_loss(x, x, m.expand(1, 3, 8, 8))
    with pytest.raises(ValueError, match="CUDA"):
        nl.make_valid_mask(torch.ones(8, 8))


# ------------------------------------------------------------------ the workspace contract
def _ws(B, H, W):
    from omnidata_amd.engine import load_library
    v = ctypes.c_int64(-1)
    return load_library().dptx_normal_workspace_bytes(B, H, W, ctypes.byref(v)), v.value


def _documented(total):
    units = (total + 3) // 4
    nblk = min((units + 1023) // 1024, 1024)
    return (24 * nblk + 255) // 256 * 256


@pytest.mark.parametrize("shape", [(1, 384, 384), (32, 384, 384), (2, 37, 53), (1, 1, 1), (3, 1, 4097), (65537, 1, 2), (1, 8192, 2048),
                                   (7, 2048, 8192)])
def test_workspace_bytes_documented(built_lib, shape):
    rc, v = _ws(*shape)
    assert rc == 0 and v == _documented(shape[0] * shape[1] * shape[2])


@pytest.mark.parametrize("shape", [(1, 4097, 4097), (1, 16, 8193), (1, 8193, 16), (0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)])
def test_workspace_bytes_rejects(built_lib, shape):
    from omnidata_amd.engine import load_library
    rc, _ = _ws(*shape)
    assert rc == -1  # DPTX_E_INVALID
    assert load_library().dptx_normal_workspace_bytes(1, 8, 8, None) == -1


def test_masked_workspace_and_host_side_argument_checks(built_lib):
    """Everything below returns before any launch: no GPU is touched."""
    from omnidata_amd.engine import load_library
    lib = load_library()
    v = ctypes.c_int64(-1)
    for n in (1, 4, 4097, 32 * 3 * 384 * 384, 1 << 40):
        assert lib.dptx_masked_workspace_bytes(n, ctypes.byref(v)) == 0 and v.value == _documented(n)
    for n in (0, -5, (1 << 40) + 1):
        assert lib.dptx_masked_workspace_bytes(n, ctypes.byref(v)) == -1
    assert lib.dptx_masked_workspace_bytes(8, None) == -1
    # H < pool, W < pool, pool < 1 and null pointers
    one = ctypes.c_void_p(256)    # never dereferenced: the shape is refused first
    for H, W, pool in ((3, 8, 4), (8, 3, 4), (8, 8, 0), (8, 8, -1)):
        assert lib.dptx_valid_mask(one, 1, H, W, pool, one, None) == -1
    assert lib.dptx_valid_mask(None, 1, 8, 8, 4, one, None) == -1
    assert lib.dptx_normal_loss(one, one, one, 1, 8, 8, 0, 10.0, one, None, one, 1 << 20, None) == -1      # no term
    assert lib.dptx_normal_loss(one, one, one, 1, 8, 8, 8, 10.0, one, None, one, 1 << 20, None) == -1      # an unknown flag
    assert lib.dptx_normal_loss(one, one, one, 1, 8, 8, 3, 10.0, one, None, one, 8, None) == -1            # workspace too small
    assert lib.dptx_masked_loss(one, None, one, 8, 0, one, None, one, 1 << 20, None) == -1                 # L1 without a target
    assert lib.dptx_masked_loss(one, one, one, 8, 2, one, None, one, 1 << 20, None) == -1                  # VALUE with one


# ------------------------------------------------------------------ the compiled unit
_asm = {}


def normal_disasm(tmp_path):
    """device assembly of normal_loss.hip alone, with the flags the library is built with"""
    if not _asm:
        from omnidata_amd.build import SOURCE_FLAGS
        out = tmp_path / "normal_loss.s"
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17"] + SOURCE_FLAGS["normal_loss.hip"] +
                           ["-S", "--cuda-device-only", "-o", str(out), os.path.join(ROOT, "omnidata_amd", "csrc", "normal_loss.hip")],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        _asm["s"] = out.read_text()
    return _asm["s"]


def test_normal_unit_built_with_the_flags_of_the_other_losses():
    from omnidata_amd.build import SOURCE_FLAGS, SOURCES
    assert "normal_loss.hip" in SOURCES
    assert SOURCE_FLAGS["normal_loss.hip"] == SOURCE_FLAGS["midas_loss.hip"] and "-packed-fp32-ops" in SOURCE_FLAGS["normal_loss.hip"]
    src = open(os.path.join(ROOT, "omnidata_amd", "csrc", "normal_loss.hip")).read()
    assert "#pragma clang fp contract(off)" in src and '#include "select.h"' in src
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("hipMalloc", "hipFree", "hipMemcpy", "Synchronize", "hipEventQuery", "hipStreamQuery", "atomic"):
        assert word not in code, word


def test_no_scratch_no_spills(tmp_path):
    s = normal_disasm(tmp_path)
    names = re.findall(r"^\s+\.name:\s+(\S+)", s, flags=re.M)
    priv = re.findall(r"^\s+\.private_segment_fixed_size:\s+(\d+)", s, flags=re.M)
    spills = re.findall(r"^\s+\.vgpr_spill_count:\s+(\d+)", s, flags=re.M)
    assert len(names) >= 12 and len(priv) == len(names) == len(spills)   # both forms of five kernels, two finalizes, pixels, mask
    assert all(int(p) == 0 for p in priv), dict(zip(names, priv))
    assert all(int(p) == 0 for p in spills), dict(zip(names, spills))


def test_no_packed_fp32_op_reads_a_high_dword_in_its_low_lane(tmp_path):
    s = normal_disasm(tmp_path)
    bad = [ln.strip() for ln in s.splitlines() if re.search(r"\bv_pk_\w+_f32\b", ln) and re.search(r"op_sel:\[[01,]*1", ln)]
    assert not bad, f"{len(bad)} packed fp32 ops with a low-lane op_sel swizzle, e.g. {bad[:3]}"
