"""GPU evaluation metrics, host side (no GPU): the workspace contract and the argument checks of the C ABI
(include/dptx.h dptx_eval_*), how eval_metrics.hip is built, and the goldens of tools/make_metrics_golden.py against
omnidata_amd.metrics on the CPU.

The criterion |d| / max(1, |v|) < 1e-6 is that of oracle/validate_metrics_vs_reference.py:64-66: fp64 on both sides, but the
reference rounds numel / valid to fp32, which is why the bound is not tighter.
"""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMAL_CASES = ("normal_odd", "normal_few", "normal_ties", "normal_nan")
DEPTH_CASES = ("depth_odd", "depth_zero_target")
CASES = NORMAL_CASES + DEPTH_CASES
THRESHOLDS = (11.25, 22.5, 30.0)
MARGIN = 1e-3
_loaded = {}


def load(name):
    """one golden of tools/make_metrics_golden.py -> dict of arrays, with keys a list of str and task a str; read once"""
    if name not in _loaded:
        z = np.load(os.path.join(ROOT, "tests", "golden", f"evalgpu_{name}.npz"))
        g = {k: z[k] for k in z.files}
        g["keys"] = [str(k) for k in g["keys"]]
        g["task"] = str(g["task"])
        _loaded[name] = g
    return _loaded[name]


def tensors(g):
    return torch.from_numpy(g["pred"]), torch.from_numpy(g["target"]), torch.from_numpy(g["mask"])


def close(got, want):
    """the 1e-6 criterion; a NaN matches a NaN only"""
    got, want = float(got), float(want)
    if np.isnan(want) or np.isnan(got):
        return bool(np.isnan(want) and np.isnan(got))
    return abs(got - want) / max(1.0, abs(want)) < 1e-6


def threshold_margin(ang, mask):
    """the smallest distance of a valid, non-NaN angle to a threshold; ang, mask: arrays of one shape"""
    a = np.asarray(ang)[np.asarray(mask, dtype=bool)]
    a = a[~np.isnan(a)]
    return min(float(np.abs(a - th).min()) for th in THRESHOLDS) if a.size else np.inf


def test_goldens_present_and_small():
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "evalgpu_*.npz")))
    assert {os.path.basename(p)[8:-4] for p in paths} >= set(CASES)
    assert all(os.path.getsize(p) < 256 << 10 for p in paths)


def test_goldens_cover_the_cases():
    o = load("normal_odd")
    assert o["pred"].shape == (3, 3, 37, 53) and o["num_valid"][0] % 2 == 1 and o["num_valid"][1] % 2 == 0 and o["num_valid"][1] > 0
    assert o["num_valid"][2] == 0 and np.isnan(o["images"][2]).all() and not np.isnan(o["images"][:2]).any()
    d = load("depth_odd")
    assert d["pred"].shape == (3, 1, 37, 53) and d["num_valid"][2] == 0 and np.isnan(d["images"][2]).all()
    f = load("normal_few")
    assert f["num_valid"].tolist() == [1, 2]
    k = f["keys"]
    for i in range(2):   # one and two valid pixels: the median is the mean
        assert abs(f["images"][i][k.index("ang_error_median")] - f["images"][i][k.index("ang_error_mean")]) < 1e-12
    t = load("normal_ties")
    valid = t["angles"][t["mask"][:, 0]]
    assert len(np.unique(valid)) * 4 < valid.size and t["batch"][t["keys"].index("ang_error_median")] == 90.0
    n = load("normal_nan")
    assert np.isnan(n["pred"]).sum() == 1 and (np.isnan(n["pred"]).any(1) & n["mask"][:, 0]).sum() == 1
    kn = n["keys"]
    for key in ("ang_error_median", "ang_error_mean", "eval_L1", "eval_mse", "ang_error_without_masking"):
        assert np.isnan(n["batch"][kn.index(key)]), key
    for key in ("percentage_within_11.25_degrees", "percentage_within_22.5_degrees", "percentage_within_30_degrees"):
        assert 0 < n["batch"][kn.index(key)] < 1
    z = load("depth_zero_target")
    outside = (z["target"][:, 0] == 0) & ~z["mask"][:, 0]
    assert outside.sum() == 1 and not ((z["target"][:, 0] == 0) & z["mask"][:, 0]).any()
    kz = z["keys"]
    assert np.isnan(z["batch"][kz.index("rel_error")])
    assert all(np.isfinite(z["batch"][i]) for i, key in enumerate(kz) if key != "rel_error")


@pytest.mark.parametrize("name", NORMAL_CASES)
def test_normal_goldens_keep_the_threshold_margin(name):
    g = load(name)
    mg = threshold_margin(g["angles"], g["mask"][:, 0])
    print(name, "threshold margin", mg)
    assert mg >= MARGIN


@pytest.mark.parametrize("name", CASES)
def test_torch_metrics_reproduce_the_goldens(name):
    """omnidata_amd.metrics on the CPU against the reference's numbers: the whole batch, and each image alone.  With a NaN
    among the valid pixels its median is finite where the reference's is NaN: that field of that case is excepted."""
    from omnidata_amd.metrics import get_metrics
    g = load(name)
    p, t, m = tensors(g)
    rows = [("batch", get_metrics(p, t, g["task"], m), g["batch"])]
    rows += [(f"image {i}", get_metrics(p[i:i + 1], t[i:i + 1], g["task"], m[i:i + 1]), g["images"][i]) for i in range(p.shape[0])]
    for what, got, want in rows:
        if got is None:
            assert np.isnan(want).all(), what
            continue
        for k, v in zip(g["keys"], want):
            print(name, what, k, got[k], v)
            if name == "normal_nan" and k == "ang_error_median" and np.isnan(v):
                assert np.isfinite(got[k])   # sort()[n // 2] does not propagate the NaN; np.median does
                continue
            assert close(got[k], v), (what, k, got[k], v)


def test_cpu_tensors_and_unknown_tasks_are_refused():
    from omnidata_amd import gpu_metrics as gm
    x = torch.rand(1, 3, 8, 8)
    m = torch.ones(1, 1, 8, 8, dtype=torch.bool)
    with pytest.raises(ValueError, match="CUDA"):
        gm.normal_metrics(x, x, m)
    with pytest.raises(ValueError, match="CUDA"):
        gm.depth_metrics(x[:, :1], x[:, :1], m)
    with pytest.raises(ValueError, match="CUDA"):
        gm.get_metrics(x, x, "normal", m)
    for task in (None, "depth", "rgb"):
        with pytest.raises(ValueError, match="task"):
            gm.get_metrics(x, x, task, m)
    with pytest.raises(ValueError, match="task"):
        gm.MetricsAccumulator("depth")


# ------------------------------------------------------------------ the workspace contract
def _ws(B, H, W):
    from omnidata_amd.engine import load_library
    v = ctypes.c_int64(-1)
    return load_library().dptx_eval_workspace_bytes(B, H, W, ctypes.byref(v)), v.value


def _documented(B, H, W):
    a = lambda x: (x + 255) // 256 * 256
    units = (H * W + 3) // 4
    nblk = min((units + 255) // 256, 1024)
    return a(8 * B * H * W) + a(72 * B * nblk) + 16384 * B + a(192 * B)


@pytest.mark.parametrize("shape", [(1, 1, 1), (32, 384, 384), (1, 8192, 2048), (3, 37, 53), (2, 200, 333), (255, 4096, 4096),
                                   (65537, 1, 2)])
def test_workspace_bytes_documented(built_lib, shape):
    rc, v = _ws(*shape)
    assert rc == 0 and v == _documented(*shape)


@pytest.mark.parametrize("shape", [(0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, 8193, 16), (1, 16, 8193), (1, 4097, 4097),
                                   (256, 4096, 4096), (1 << 20, 64, 64)])
def test_workspace_bytes_rejects(built_lib, shape):
    """B = 0, a side over 8192, H*W over 2^24, B*H*W >= 2^32 (exactly 2^32 twice), a null `bytes`"""
    from omnidata_amd.engine import load_library
    rc, _ = _ws(*shape)
    assert rc == -1  # DPTX_E_INVALID
    assert load_library().dptx_eval_workspace_bytes(1, 8, 8, None) == -1


def test_host_side_argument_checks(built_lib):
    """Everything below returns before any launch: no GPU is touched."""
    from omnidata_amd.engine import load_library
    lib = load_library()
    one = ctypes.c_void_p(256)    # never dereferenced: the arguments are refused first
    _, need = _ws(1, 8, 8)
    for fn in (lib.dptx_eval_normal, lib.dptx_eval_depth):
        for null in range(5):     # pred, target, mask, out, ws
            ptrs = [one] * 5
            ptrs[null] = None
            assert fn(ptrs[0], ptrs[1], ptrs[2], 1, 8, 8, 0, ptrs[3], ptrs[4], 1 << 20, None) == -1, null
        for flags in (2, 3, 4, -1, 1 << 16):                                                  # an unknown flag
            assert fn(one, one, one, 1, 8, 8, flags, one, one, 1 << 20, None) == -1, flags
        for flags in (0, 1):
            assert fn(one, one, one, 1, 8, 8, flags, one, one, need - 1, None) == -1          # workspace too small
            assert fn(one, one, one, 0, 8, 8, flags, one, one, 1 << 20, None) == -1           # an unsupported shape
            assert fn(one, one, one, 1, 8193, 8, flags, one, one, 1 << 40, None) == -1
    assert lib.dptx_eval_normal_pixels(None, one, 1, 8, 8, one, None) == -1
    assert lib.dptx_eval_normal_pixels(one, None, 1, 8, 8, one, None) == -1
    assert lib.dptx_eval_normal_pixels(one, one, 1, 8, 8, None, None) == -1
    assert lib.dptx_eval_normal_pixels(one, one, 0, 8, 8, one, None) == -1
    assert lib.dptx_eval_normal_pixels(one, one, 1 << 20, 64, 64, one, None) == -1


# ------------------------------------------------------------------ the unit
def test_eval_unit_built_with_the_flags_of_the_normal_loss():
    from omnidata_amd.build import SOURCE_FLAGS, SOURCES
    assert "eval_metrics.hip" in SOURCES
    assert SOURCE_FLAGS["eval_metrics.hip"] == SOURCE_FLAGS["normal_loss.hip"] and "-packed-fp32-ops" in SOURCE_FLAGS["eval_metrics.hip"]
    src = open(os.path.join(ROOT, "omnidata_amd", "csrc", "eval_metrics.hip")).read()
    assert "#pragma clang fp contract(off)" in src and '#include "select.h"' in src


# ------------------------------------------------------------------ the select, restated
def d2key(a):
    """order-preserving uint64 keys of fp64 values (eval_metrics.hip d2key); -0.0 and +0.0 are one key"""
    u = np.where(a == 0, 0.0, a).astype(np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def key2d(k):
    u = (k & ~(1 << 63)) if k >> 63 else ~k & ((1 << 64) - 1)
    return float(np.array([u], dtype=np.uint64).view(np.float64)[0])


def restated_median(values):
    """The two-rank radix select as eval_metrics.hip runs it, in numpy: 8 passes of 8 bits, most significant digit first;
    n is the total of pass 0's histogram, the ranks are (n - 1) // 2 and n // 2; the state before pass q comes from the
    state before pass q - 1 and that pass's histograms, one histogram serving both ranks while their prefixes agree."""
    keys = [int(k) for k in d2key(np.asarray(values, dtype=np.float64))]
    hist = np.zeros((8, 2, 256), np.int64)
    for k in keys:
        hist[0, 0, k >> 56] += 1
    state = {}

    def state_before(q):
        pre, rank = ([0, 0], [0, 0]) if q == 1 else (list(state[q - 1][0]), list(state[q - 1][1]))
        h = (hist[q - 1, 0], hist[q - 1, 0] if pre[0] == pre[1] else hist[q - 1, 1])
        inc = [np.cumsum(x) for x in h]
        n = int(inc[0][255])
        if q == 1:
            rank = [(n - 1) // 2 if n else 0, n // 2]
        out = ([p << 8 for p in pre], [0, 0])
        for a in range(2):
            for t in range(256):
                ex = int(inc[a][t]) - int(h[a][t])
                if ex <= rank[a] < int(inc[a][t]):
                    out[0][a], out[1][a] = (pre[a] << 8) | t, rank[a] - ex
        return out

    for q in range(1, 8):
        pre, _ = state[q] = state_before(q)
        shift = 64 - 8 * (q + 1)
        for k in keys:
            top, digit = k >> (shift + 8), (k >> shift) & 255
            if top == pre[0]:
                hist[q, 0, digit] += 1
            if pre[0] != pre[1] and top == pre[1]:
                hist[q, 1, digit] += 1
    pre, _ = state_before(8)
    return (key2d(pre[0]) + key2d(pre[1])) * 0.5


def test_restated_select_is_np_median():
    """odd and even counts, one and two values, ties, zeros of both signs: bit for bit np.median"""
    rng = np.random.default_rng(0)
    cases = []
    for name in ("normal_few", "normal_ties", "normal_nan"):
        g = load(name)
        a, m = g["angles"], g["mask"][:, 0]
        cases += [a[m]] + [a[i][m[i]] for i in range(a.shape[0])]
    for n in (1, 2, 3, 4, 7, 100, 101):
        v = rng.random(n) * 180
        v[:n // 3] = v[0]
        cases.append(v)
    cases += [np.array([0.0, -0.0, 0.0, 5.0]), np.array([-0.0, 0.0])]
    for v in cases:
        v = v[~np.isnan(v)]
        got, want = restated_median(v), float(np.median(v))
        assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (v.size, got, want)
