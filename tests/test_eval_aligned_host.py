"""Scale-and-shift-aligned depth evaluation (include/dptx.h dptx_eval_depth_aligned), the part that needs no GPU: the goldens
of tools/make_eval_aligned_golden.py, the restatement pinned to them on the CPU, the workspace formula and the host-side
argument checks."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

import eval_aligned_restatement as rs
from gpu_util import ulps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "evalaligned_*.npz")))
IDS = [os.path.basename(p)[12:-4] for p in GOLDEN]
MARGIN = 1e-5        # relative distance of every valid ratio from a delta threshold
INVALID = -1         # DPTX_E_INVALID


def crit(got, want):
    """the project's metric criterion: |d| / max(1, |v|)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def load(path):
    z = np.load(path)
    g = {k: (torch.from_numpy(z[k]) if z[k].dtype.kind in "fb" else z[k]) for k in z.files}
    g["keys"] = [str(k) for k in z["keys"]]
    return g


def golden_stats(g, which):
    """the stored reference numbers of one run ('32' or '64') in the restatement's form"""
    s, c = g["stats" + which], g["coeffs" + which]
    return {"t_p": s[:, 0], "t_g": s[:, 1], "s_p": s[:, 2], "s_g": s[:, 3], "scale": c[:, 0], "shift": c[:, 1]}


def reference_rows(g, align):
    """[B + 1, 15] with the reference's numbers at the fields it has and NaN elsewhere"""
    B = g["pred"].shape[0]
    out = np.full((B + 1, len(rs.FIELDS)), np.nan)
    for k, name in enumerate(g["keys"]):
        out[:B, rs.FIELDS.index(name)] = g[align + "_images"][:, k].numpy()
        out[B, rs.FIELDS.index(name)] = float(g[align + "_batch"][k])
    return out


def test_goldens_are_present_and_small():
    assert len(GOLDEN) == 3 and set(IDS) == {"odd", "vec", "blocks"}
    shapes = {tuple(np.load(p)["pred"].shape) for p in GOLDEN}
    assert shapes == {(2, 1, 37, 53), (3, 1, 48, 64), (2, 1, 96, 130)}
    biggest = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "evalgpu_*.npz")))
    assert all(os.path.getsize(p) <= biggest for p in GOLDEN)


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
@pytest.mark.parametrize("align", ["lstsq", "median"])
def test_goldens_keep_the_delta_margin(path, align):
    g = load(path)
    al = rs.aligned(g["pred"], align, golden_stats(g, "32"), True)
    mg = rs.ratio_margin(al, g["target"], g["mask"])
    print(f"\n[{os.path.basename(path)} {align}] delta margin {mg:.2e}")
    assert mg >= MARGIN


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_restatement_reproduces_the_goldens(path):
    """The bars of the GPU test: coefficients within 1 fp32 ulp of the reference's fp64 run, rows within 1e-6 (criterion) of
    the reference's row, which it composed with its fp32 run's coefficients."""
    g = load(path)
    st = rs.stats(g["pred"], g["target"], g["mask"])
    want = golden_stats(g, "64")
    for k in ("t_p", "t_g"):
        assert ulps(st[k], want[k]).max() == 0, k
    for k in ("s_p", "s_g", "scale", "shift"):
        assert ulps(st[k], want[k]).max() <= 1, (k, st[k], want[k])
    for align in ("lstsq", "median"):
        rows = rs.rows(rs.aligned(g["pred"], align, st, True), g["target"], g["mask"]).numpy()
        ref = reference_rows(g, align)
        have = ~np.isnan(ref)
        assert have[:, 1:8].all() and not have[:, 8:].any()
        d = crit(rows[have], ref[have])
        print(f"\n[{os.path.basename(path)} {align}] restatement vs reference rows: {d:.2e}")
        assert d < 1e-6
        assert np.array_equal(rows[:, 0], np.append(g["mask"].reshape(g["mask"].shape[0], -1).sum(1).numpy(), int(g["mask"].sum())))
        # the reference's own fp32-sum coefficients against its fp64 ones, through the same rows: the room under the bar
        own = rs.rows(rs.aligned(g["pred"], align, golden_stats(g, "64"), True), g["target"], g["mask"]).numpy()
        print(f"    reference fp32-run vs fp64-run coefficients, rows: {crit(own[have], ref[have]):.2e}")


def test_restatement_fields_8_to_14_on_a_hand_case():
    """a_e / t_e = 2 on two pixels, 1 on one, and a floor: the definitions of the seven benchmark fields by hand"""
    al = torch.tensor([0.2, 0.4, 0.5, 0.0, 9.0]).view(1, 1, 1, 5)
    t = torch.tensor([0.1, 0.2, 0.5, 0.0, 1.0]).view(1, 1, 1, 5)
    m = torch.tensor([True, True, True, True, False]).view(1, 1, 1, 5)
    r = rs.rows(al, t, m, min_depth=1e-3)[0].numpy()
    a, g = np.float32([0.2, 0.4, 0.5, 1e-3]).astype(np.float64), np.float32([0.1, 0.2, 0.5, 1e-3]).astype(np.float64)
    d = a - g
    want = [np.mean(np.abs(d) / g), np.mean(d * d / g), np.sqrt(np.mean(d * d)), np.sqrt(np.mean(np.log(a / g) ** 2)), 0.5, 0.5, 0.5]
    assert r[0] == 4 and np.allclose(r[8:], want, rtol=1e-12, atol=0)
    r2 = rs.rows(al * 0.99, t, m)[0].numpy()   # ratio 1.98 >= 1.953125 still outside delta3; 1 / 0.99 inside delta1
    assert list(r2[12:]) == [0.5, 0.5, 0.5]
    r3 = rs.rows(al * 0.97, t, m)[0].numpy()   # ratio 1.94 < 1.953125
    assert list(r3[12:]) == [0.5, 0.5, 1.0]


def nblk_eval(H, W):
    return min(-(-(-(-H * W // 4)) // 256), 1024)


def header_formula(B, H, W, midas_bytes):
    """include/dptx.h: *bytes = A(120 B nblk) + A(32 B) + M"""
    A = lambda x: (x + 255) // 256 * 256
    return A(120 * B * nblk_eval(H, W)) + A(32 * B) + midas_bytes


def test_workspace_formula_is_the_headers(built_lib):
    from omnidata_amd.engine import load_library
    lib = load_library()
    text = open(os.path.join(ROOT, "include", "dptx.h")).read()
    assert re.search(r"\*bytes = A\(120 B nblk\) \+ A\(32 B\) \+ M", text)
    for B, H, W in ((1, 1, 1), (2, 37, 53), (3, 48, 64), (2, 96, 130), (32, 384, 384), (1, 4096, 4096), (5, 1, 8192)):
        got, mid = C.c_int64(), C.c_int64()
        assert lib.dptx_eval_aligned_workspace_bytes(B, H, W, C.byref(got)) == 0
        assert lib.dptx_midas_workspace_bytes(B, H, W, 1, C.byref(mid)) == 0
        assert got.value == header_formula(B, H, W, mid.value), (B, H, W)


def test_workspace_call_rejects_bad_shapes_and_null(built_lib):
    from omnidata_amd.engine import load_library
    lib = load_library()
    b = C.c_int64()
    assert lib.dptx_eval_aligned_workspace_bytes(2, 37, 53, None) == INVALID
    for shape in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 8193, 1), (1, 1, 8193), (1, 8192, 4096), (256, 4096, 4096), (-1, 8, 8)):
        assert lib.dptx_eval_aligned_workspace_bytes(*shape, C.byref(b)) == INVALID, shape


def test_argument_checks_need_no_device(built_lib):
    """Every call below carries one invalid argument, so it returns before anything is launched: the pointers are host
    buffers that are never read."""
    from omnidata_amd.engine import load_library
    lib = load_library()
    B, H, W = 2, 8, 8
    need = C.c_int64()
    assert lib.dptx_eval_aligned_workspace_bytes(B, H, W, C.byref(need)) == 0
    bufs = {k: (C.c_char * n)() for k, n in (("pred", 4 * B * H * W), ("target", 4 * B * H * W), ("mask", B * H * W),
                                               ("out", 8 * 15 * (B + 1)), ("coeffs", 8 * B), ("ws", need.value + 16))}
    ptr = {k: C.cast(v, C.c_void_p) for k, v in bufs.items()}

    def call(align=1, flags=1, min_depth=1e-3, shape=(B, H, W), ws_bytes=need.value, ws_off=0, **null):
        p = {k: (None if k in null else v) for k, v in ptr.items()}
        ws = None if p["ws"] is None else C.c_void_p(p["ws"].value + ws_off)
        return lib.dptx_eval_depth_aligned(p["pred"], p["target"], p["mask"], *shape, align, flags, C.c_float(min_depth), p["out"],
                                           p["coeffs"], None, ws, ws_bytes, None)

    for name in ("pred", "target", "mask", "out", "coeffs", "ws"):
        assert call(**{name: True}) == INVALID, name
    for align in (0, 3, 4, -1):
        assert call(align=align) == INVALID, align
    for flags in (2, 3, -1, 1 << 16):
        assert call(flags=flags) == INVALID, flags
    for md in (0.0, -1e-3, float("inf"), float("nan"), -float("inf")):
        assert call(min_depth=md) == INVALID, md
    assert call(ws_bytes=need.value - 1) == INVALID and call(ws_bytes=0) == INVALID
    assert call(shape=(0, H, W)) == INVALID and call(shape=(B, 8193, W)) == INVALID
    assert call(ws_off=4) == INVALID   # the workspace holds fp64 sums


def test_header_and_abi_agree(built_lib):
    from omnidata_amd.engine import ABI
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dptx.h")).read(), flags=re.S)
    names = {n for n, _, _ in ABI}
    for sym in ("dptx_eval_aligned_workspace_bytes", "dptx_eval_depth_aligned"):
        assert re.search(rf"\b{sym}\s*\(", text) and sym in names
    args = {n: a for n, _, a in ABI}
    assert len(args["dptx_eval_depth_aligned"]) == 15 and args["dptx_eval_depth_aligned"][8] is C.c_float
    for name, value in (("ALIGN_LSTSQ", 1), ("ALIGN_MEDIAN", 2), ("ALIGNED_CLAMP", 1), ("ALIGNED_FIELDS", 15)):
        assert re.search(rf"#define DPTX_EVAL_{name} {value}\b", text), name
    from omnidata_amd import gpu_metrics as gm
    assert gm.ALIGNED_DEPTH_FIELDS == rs.FIELDS and gm._ALIGN == {"lstsq": 1, "median": 2} and gm.ALIGNED_CLAMP == 1
