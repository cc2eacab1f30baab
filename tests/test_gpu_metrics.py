"""GPU evaluation metrics (omnidata_amd/gpu_metrics.py, csrc/eval_metrics.hip) against the reference's goldens
(tools/make_metrics_golden.py, oracle/validate_metrics_vs_reference.py) and omnidata_amd.metrics on the CPU.  pytest -m gpu.

Bounds.  Metrics: |d| / max(1, |v|) < 1e-6, the criterion of oracle/validate_metrics_vs_reference.py:64-66 (fp64 on both
sides; the reference rounds numel / valid to fp32); a NaN matches a NaN only.  The `<=` thresholds can flip on a last-bit
difference of acos, so every case keeps its valid angles 1e-3 degrees away from 11.25, 22.5 and 30: the goldens by the
tool's assertion (checked again in tests/test_metrics_gpu_host.py), the case made here by an assertion of its own.
Per-pixel angles: |d| <= 1e-5 degrees.  With contraction off the two sides differ by at most about 12 ulp of the cosine
(1.4e-15: the order of a three-term sum, and acos), which moves the angle by at most sqrt(2 * 1.4e-15) rad = 3e-6 degrees at
cos -> +-1 and by less elsewhere: 1e-5 carries a 3x margin.
The median is exact: it equals np.median of the kernel's own per-pixel angles over the mask bit for bit.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from omnidata_amd import gpu_metrics as gm
from omnidata_amd import metrics as tm
from oracle.validate_metrics_vs_reference import make_case
from test_metrics_gpu_host import DEPTH_CASES, MARGIN, NORMAL_CASES, close, load, tensors, threshold_margin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {"normal": gm.NORMAL_FIELDS, "depth_zbuffer": gm.DEPTH_FIELDS}
BIG_SEED = {"normal": 48, "depth_zbuffer": 7}   # normal: picked on the CPU, its valid angles stay 3.4e-3 degrees off the thresholds
_big = {}


def rows(task, p, t, m, per_image):
    """the kernel's rows as a numpy array [rows, fields]"""
    return gm._rows(task, p.cuda(), t.cuda(), m.cuda(), per_image).cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def check_row(task, row, want, count, what):
    """row [fields] of the kernel against want {name: value} (None or all-NaN: an empty row) with the 1e-6 criterion"""
    fields = FIELDS[task]
    assert row[0] == count, (what, row[0], count)
    if count == 0:
        assert np.isnan(row[1:]).all(), (what, row)
        return
    for k, name in enumerate(fields[1:], 1):
        print(what, name, repr(float(row[k])), repr(float(want[name])))
        assert close(row[k], want[name]), (what, name, row[k], want[name])


def big_case(task, seed=None):
    """B = 2, 200 x 333 (66600 pixels an image: 66 blocks of 253 units, the last one short), a random 80 % mask.  Normals
    are raw vectors in [-1, 1]^3 in independent directions, so that the angles spread over (0, 180) and few lie near a
    threshold; computed once"""
    if seed is not None or task not in _big:
        g = torch.Generator().manual_seed(1000 + (BIG_SEED[task] if seed is None else seed))
        B, H, W = 2, 200, 333
        if task == "normal":
            t = torch.randn(B, 3, H, W, generator=g)
            t = t / t.norm(dim=1, keepdim=True)
            p = torch.randn(B, 3, H, W, generator=g)
            p = p / p.norm(dim=1, keepdim=True) * (0.5 + torch.rand(B, 1, H, W, generator=g))
        else:
            t = torch.rand(B, 1, H, W, generator=g) * 0.9 + 0.05
            p = (t + 0.05 * torch.randn(B, 1, H, W, generator=g)).clamp(min=0.0)
        m = torch.rand(B, 1, H, W, generator=g) < 0.8
        if seed is not None:
            return p, t, m
        _big[task] = (p, t, m)
    return _big[task]


def cpu_angles(p, t):
    p, t = p.double(), t.double()
    cos = ((p * t).sum(1) / (p.norm(dim=1) * t.norm(dim=1)).clamp(min=1e-8)).clamp(-1.0, 1.0)
    return torch.acos(cos) * (180.0 / np.pi)


def normal_inputs(name):
    """every normal case by name -> pred, target, mask (CPU)"""
    if name in NORMAL_CASES:
        return tensors(load(name))
    if name == "big":
        return big_case("normal")
    return make_case(int(name[-1]), "normal")


ALL_NORMAL = NORMAL_CASES + ("seed0", "seed1", "big")


# ------------------------------------------------------------------ 1. the goldens of oracle/validate_metrics_vs_reference.py
@pytest.mark.parametrize("task", ["normal", "depth_zbuffer"])
@pytest.mark.parametrize("seed", [0, 1])
def test_existing_goldens_batch_row(task, seed):
    z = np.load(os.path.join(ROOT, "tests", "golden", f"metrics_{task}_seed{seed}.npz"))
    want = {str(k): float(v) for k, v in zip(z["keys"], z["values"])}
    p, t, m = make_case(seed, task)
    check_row(task, rows(task, p, t, m, False)[0], want, int(m.sum()), f"{task} seed{seed}")


# ------------------------------------------------------------------ 2, 3, 4, 8. the goldens of tools/make_metrics_golden.py
@pytest.mark.parametrize("name", NORMAL_CASES + DEPTH_CASES)
def test_goldens_batch_and_per_image_rows(name):
    """normal_odd / depth_odd: 37 x 53, an odd count, an even count and an empty image (count 0, NaN elsewhere);
    normal_few: one and two valid pixels; normal_ties: few distinct angles; normal_nan: a NaN inside the mask makes the
    mean, the median, L1, MSE and the unmasked mean NaN and leaves the percentages; depth_zero_target: target == 0 outside
    the mask makes rel_error NaN alone"""
    g = load(name)
    task = g["task"]
    p, t, m = tensors(g)
    check_row(task, rows(task, p, t, m, False)[0], dict(zip(g["keys"], g["batch"])), int(g["num_valid"].sum()), f"{name} batch")
    per = rows(task, p, t, m, True)
    assert per.shape == (p.shape[0], len(FIELDS[task]))
    for i in range(p.shape[0]):
        check_row(task, per[i], dict(zip(g["keys"], g["images"][i])), int(g["num_valid"][i]), f"{name} image {i}")


def test_one_and_two_valid_pixels_median_is_the_mean():
    g = load("normal_few")
    per = rows("normal", *tensors(g), True)
    k = gm.NORMAL_FIELDS
    mean, median = per[:, k.index("ang_error_mean")], per[:, k.index("ang_error_median")]
    print("mean", mean.tolist(), "median", median.tolist())
    assert per[:, 0].tolist() == [1.0, 2.0]
    assert (np.abs(mean - median) <= 1e-12 * mean).all()


def test_ties_median_is_exactly_90():
    g = load("normal_ties")
    got = rows("normal", *tensors(g), False)[0]
    assert got[gm.NORMAL_FIELDS.index("ang_error_median")] == 90.0


# ------------------------------------------------------------------ 5. per-pixel angles
@pytest.mark.parametrize("name", NORMAL_CASES)
def test_per_pixel_angles(name):
    g = load(name)
    p, t, _ = tensors(g)
    got = gm.normal_angles(p.cuda(), t.cuda()).cpu().numpy()
    want = g["angles"]
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want))
    d = np.nanmax(np.abs(got - want))
    print(name, "max |angle - reference angle| (degrees):", d)
    assert d <= 1e-5


# ------------------------------------------------------------------ 6. the median is exact
@pytest.mark.parametrize("name", ALL_NORMAL)
def test_median_is_np_median_of_the_kernels_own_angles(name):
    p, t, m = normal_inputs(name)
    ang = gm.normal_angles(p.cuda(), t.cuda()).cpu().numpy()
    mk = m[:, 0].numpy()
    k = gm.NORMAL_FIELDS.index("ang_error_median")
    batch = rows("normal", p, t, m, False)[0]
    per = rows("normal", p, t, m, True)
    with np.errstate(all="ignore"):
        cases = [("batch", batch, ang[mk])] + [(f"image {i}", per[i], ang[i][mk[i]]) for i in range(p.shape[0])]
        for what, row, valid in cases:
            want = np.median(valid) if valid.size else np.nan
            print(name, what, "median", repr(float(row[k])), "np.median", repr(float(want)), "n", valid.size)
            assert row[0] == valid.size
            assert (np.isnan(want) and np.isnan(row[k])) or same_bits(row[k], want), (what, row[k], want)


# ------------------------------------------------------------------ 7. several blocks and a remainder
@pytest.mark.parametrize("task", ["normal", "depth_zbuffer"])
def test_several_blocks_against_torch_metrics_on_the_cpu(task):
    p, t, m = big_case(task)
    if task == "normal":
        mg = threshold_margin(cpu_angles(p, t).numpy(), m[:, 0].numpy())
        print("threshold margin", mg)
        assert mg >= MARGIN
    check_row(task, rows(task, p, t, m, False)[0], tm.get_metrics(p, t, task, m), int(m.sum()), f"{task} batch")
    per = rows(task, p, t, m, True)
    for i in range(p.shape[0]):
        check_row(task, per[i], tm.get_metrics(p[i:i + 1], t[i:i + 1], task, m[i:i + 1]), int(m[i].sum()), f"{task} image {i}")


# ------------------------------------------------------------------ 9. reproducibility and invariance
@pytest.mark.parametrize("task,name", [("normal", "normal_odd"), ("depth_zbuffer", "depth_odd"), ("normal", "big"), ("depth_zbuffer", "big")])
def test_bitwise_same_call_twice_and_batch_invariance(task, name):
    """The same call twice gives the same bits; row i of a per-image call equals the single row of a B = 1 call on image i,
    with and without DPTX_EVAL_PER_IMAGE; the image's place in the batch does not matter."""
    p, t, m = big_case(task) if name == "big" else tensors(load(name))
    for per_image in (False, True):
        assert same_bits(rows(task, p, t, m, per_image), rows(task, p, t, m, per_image))
    per = rows(task, p, t, m, True)
    for i in range(p.shape[0]):
        one = (p[i:i + 1], t[i:i + 1], m[i:i + 1])
        assert same_bits(per[i], rows(task, *one, False)[0]), i
        assert same_bits(per[i], rows(task, *one, True)[0]), i
    flipped = rows(task, p.flip(0), t.flip(0), m.flip(0), True)
    assert same_bits(flipped, per[::-1])


@pytest.mark.parametrize("task", ["normal", "depth_zbuffer"])
def test_bitwise_cached_workspaces_carry_no_stale_state(task):
    """case 2, then case 7, then case 2 again: the third result is the first.  Workspaces are cached per shape, so the calls
    that really follow one another on ONE workspace are those on other data of case 2's shape in between: a permutation of
    its pixels with another mask (other keys, other histograms, other counts, an image that is no longer empty)."""
    small = tensors(load("normal_odd" if task == "normal" else "depth_odd"))
    big = big_case(task)
    g = torch.Generator().manual_seed(5)
    perm = torch.randperm(small[0][0, 0].numel(), generator=g)
    shuffled = lambda x: x.flatten(2)[:, :, perm].reshape(x.shape).flip(0).contiguous()
    other = (shuffled(small[1]), shuffled(small[0]), torch.rand(small[2].shape, generator=g) < 0.5)
    first = [rows(task, *small, per_image) for per_image in (False, True)]
    between = [rows(task, *big, per_image) for per_image in (False, True)]
    same_shape = [rows(task, *other, per_image) for per_image in (False, True)]
    again = [rows(task, *small, per_image) for per_image in (False, True)]
    assert same_bits(first[0], again[0]) and same_bits(first[1], again[1])
    assert not same_bits(first[0], same_shape[0]) and (same_shape[1][:, 0] > 0).all()
    assert same_bits(between[0], rows(task, *big, False))
    assert same_bits(same_shape[1], rows(task, *other, True))


@pytest.mark.parametrize("task", ["normal", "depth_zbuffer"])
def test_bitwise_same_on_misaligned_pointers(task):
    """24 x 32 and 200 x 333 have H*W % 4 == 0: 16-byte loads.  The same tensors 4 bytes further on take the scalar path over
    the same units, and give the same bits."""
    for p, t, m in (make_case(0, task), big_case(task)):
        def shifted(x):
            buf = torch.empty(x.numel() + 1, dtype=x.dtype, device="cuda")
            buf[1:] = x.flatten().cuda()
            v = buf[1:].view(x.shape)
            assert v.is_contiguous() and v.data_ptr() % 16 != 0
            return v
        for per_image in (False, True):
            want = rows(task, p, t, m, per_image)
            got = gm._rows(task, shifted(p), shifted(t), m.cuda(), per_image).cpu().numpy()
            assert same_bits(got, want), per_image


# ------------------------------------------------------------------ 10. inputs
@pytest.mark.parametrize("task", ["normal", "depth_zbuffer"])
def test_input_contract(task):
    p, t, m = make_case(1, task)
    C = p.shape[1]
    fn = gm.normal_metrics if task == "normal" else gm.depth_metrics
    pc, tc, mc = p.cuda(), t.cuda(), m.cuda()
    want = fn(pc, tc, mc)
    assert set(want) == set(tm.get_metrics(p, t, task, m)) | {"num_valid"}
    assert all(v.dtype == torch.float64 and v.is_cuda and v.dim() == 0 for v in want.values())
    per = fn(pc, tc, mc, per_image=True)
    assert all(v.shape == (p.shape[0],) and v.dtype == torch.float64 and v.is_cuda for v in per.values())
    # 16-bit inputs: the result on their .float() copies, bit for bit
    for dt in (torch.bfloat16, torch.float16):
        got = fn(pc.to(dt), tc.to(dt), mc)
        ref = fn(pc.to(dt).float(), tc.to(dt).float(), mc)
        assert all(same_bits(got[k].cpu().numpy(), ref[k].cpu().numpy()) for k in ref), dt
    # a mask with C channels (here 3 even for depth is refused): channel 0 is used
    wide = torch.cat([mc] + [~mc] * (C - 1), 1) if C > 1 else mc
    got = fn(pc, tc, wide)
    assert all(same_bits(got[k].cpu().numpy(), want[k].cpu().numpy()) for k in want)
    # a non-contiguous prediction
    nc = pc.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) if C > 1 else pc.transpose(2, 3).contiguous().transpose(2, 3)
    assert not nc.is_contiguous() and torch.equal(nc, pc)
    got = fn(nc, tc, mc)
    assert all(same_bits(got[k].cpu().numpy(), want[k].cpu().numpy()) for k in want)
    # refusals, before any launch
    with pytest.raises(ValueError, match="CUDA"):
        fn(p, tc, mc)
    with pytest.raises(ValueError, match="CUDA"):
        fn(pc, tc, m)
    with pytest.raises(ValueError, match="mismatch"):
        fn(pc, tc[:, :, :-1], mc)
    with pytest.raises(ValueError, match="mask must be"):
        fn(pc, tc, mc[:, :, :, :-1])
    with pytest.raises(ValueError, match="mask must be"):
        fn(pc, tc, torch.cat([mc, mc], 1))
    with pytest.raises(ValueError, match="bool"):
        fn(pc, tc, mc.float())
    with pytest.raises(ValueError, match=r"\[B,"):
        fn(pc[:, :1] if C > 1 else pc.expand(-1, 3, -1, -1), tc[:, :1] if C > 1 else tc.expand(-1, 3, -1, -1), mc)
    with pytest.raises(ValueError, match="fp32, fp16 or bf16"):
        fn(pc.double(), tc, mc)
    with pytest.raises(ValueError, match="task"):
        gm.get_metrics(pc, tc, "rgb", mc)
    with pytest.raises(ValueError, match="task"):
        gm.get_metrics(pc, tc, None, mc)
    # get_metrics: the reference's shape
    got = gm.get_metrics(pc, tc, task, mc)
    ref = tm.get_metrics(p, t, task, m)
    assert set(got) == set(ref) and all(isinstance(v, float) for v in got.values())
    assert all(close(got[k], ref[k]) for k in ref)
    assert gm.get_metrics(pc, tc, task, torch.zeros_like(mc)) is None


@pytest.mark.parametrize("task,name", [("normal", "normal_odd"), ("depth_zbuffer", "depth_odd")])
def test_accumulator_over_two_batches(task, name):
    """mean and sample std (divisor n - 1) of the concatenated per-image rows, empty images skipped"""
    a = tensors(load(name))               # three images, the last one empty
    b = make_case(0, task)                # two images of another shape
    acc = gm.MetricsAccumulator(task)
    acc.update(*(x.cuda() for x in a))
    acc.update(*(x.cuda() for x in b))
    got = acc.compute()
    allrows = np.concatenate([rows(task, *a, True), rows(task, *b, True)])
    kept = allrows[allrows[:, 0] > 0]
    assert len(kept) == 4 and got["num_images"] == 4
    for k, name_ in enumerate(FIELDS[task]):
        mean, std = got[name_]
        wm, ws = kept[:, k].mean(), kept[:, k].std(ddof=1)
        print(name_, mean, wm, std, ws)
        # sums of four values of one sign: the mean to a few ulp; the variance from sum and sum of squares loses
        # mean^2 / variance of the 2^-53 relative rounding, below 1e-9 for these spreads
        assert abs(mean - wm) <= 1e-14 * abs(wm) and abs(std - ws) <= 1e-9 * max(abs(wm), ws)
    empty = gm.MetricsAccumulator(task)
    empty.update(a[0][2:].cuda(), a[1][2:].cuda(), a[2][2:].cuda())
    out = empty.compute()
    assert out["num_images"] == 0 and all(np.isnan(out[n][0]) and np.isnan(out[n][1]) for n in FIELDS[task])


# ------------------------------------------------------------------ 11. tools/eval_checkpoint.py --device-metrics
def test_eval_checkpoint_device_metrics_match_the_default_path(tmp_path, capsys):
    """on the synthetic Lightning checkpoint of tests/test_gpu_eval_checkpoint.py: same weights, images and ground truth,
    the metrics of the two paths agree within the 1e-6 criterion"""
    from PIL import Image
    from omnidata_amd.weights import random_state_dict
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eval_checkpoint as ec
    sd = random_state_dict(0, 3)
    ckpt = tmp_path / "omnidata_dpt_normal_v2.ckpt"
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}, "epoch": 3}, ckpt)
    img_dir, gt_dir = tmp_path / "img", tmp_path / "gt"
    img_dir.mkdir()
    gt_dir.mkdir()
    rng = np.random.default_rng(0)
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (400 + 16 * i, 500, 3), dtype=np.uint8)).save(img_dir / f"im{i}.png")
        n = rng.normal(size=(400 + 16 * i, 500, 3)).astype(np.float32)
        np.save(gt_dir / f"im{i}.npy", n / np.linalg.norm(n, axis=2, keepdims=True))
    m = np.zeros((416, 500), np.uint8)
    m[50:300, 60:400] = 255
    Image.fromarray(m).save(gt_dir / "im1_mask.png")
    args = ["--task", "normal", "--ckpt", str(ckpt), "--images", str(img_dir), "--gt", str(gt_dir), "--dtypes", "bf16", "--batch", "2"]
    reports = {}
    for flag in ([], ["--device-metrics"]):
        out = tmp_path / f"report{len(flag)}.json"
        ec.main(args + flag + ["--out", str(out)])
        reports[len(flag)] = json.loads(out.read_text())["dtypes"]["bf16"]
    capsys.readouterr()
    ref, dev = reports[0], reports[1]
    assert ref["metrics_images"] == dev["metrics_images"] == 2
    assert set(ref["metrics"]) == set(dev["metrics"]) and len(ref["metrics"]) == 8
    for k, v in ref["metrics"].items():
        print(k, v, dev["metrics"][k])
        assert close(dev["metrics"][k], v), (k, dev["metrics"][k], v)
