"""Writes tests/golden/evalgpu_*.npz: inputs and the reference's evaluation metrics for them, computed on the CPU.

    python tools/make_metrics_golden.py --omnidata <checkout of EPFL-VILAB/omnidata>

Loads paper_code/evaluation_metrics.py from that checkout at run time (it imports torchvision, pandas and tqdm at the top
without using them in get_metrics; missing ones are stubbed, as oracle/validate_metrics_vs_reference.py does).  Nothing of
the checkout is copied here.

Every file holds task, pred, target [B,C,H,W] fp32, mask [B,1,H,W] bool, keys (the reference's names, sorted), batch
[len(keys)] fp64 = get_metrics on the whole batch, images [B][len(keys)] fp64 = one get_metrics call per image (a row of
NaN where it returns None), num_valid [B], and for the normal task angles [B,H,W] fp64: the per-pixel angular error in
degrees by the reference's formula (:36-43), pinned here to the reference's own mean and median of them.

For every normal case the tool ASSERTS that no valid pixel's angle lies within MARGIN = 1e-3 degrees of 11.25, 22.5 or 30,
so that the `<=` thresholds cannot flip on a last-bit difference of acos.  Random cases take the first seed for which that
holds; the `ties` case, whose small integer vectors do put angles exactly on a threshold, masks such pixels out.
"""
from __future__ import annotations

import argparse
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
THRESHOLDS = (11.25, 22.5, 30.0)
MARGIN = 1e-3


def load_reference(checkout: str):
    for name in ("torchvision", "pandas", "tqdm"):
        try:
            __import__(name)
        except Exception:
            mod = types.ModuleType(name)
            if name == "tqdm":
                mod.tqdm = lambda x, *a, **k: x
            sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("reference_evaluation_metrics", os.path.join(checkout, "paper_code", "evaluation_metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def angles(pred, target):
    """[B,H,W] fp64 degrees: the formula of :36-43 on the .double() inputs"""
    p, t = pred.double(), target.double()
    w12 = (p * t).sum(1)
    w1, w2 = (p * p).sum(1).sqrt(), (t * t).sum(1).sqrt()
    return torch.acos((w12 / (w1 * w2).clamp(min=1e-8)).clamp(-1.0, 1.0)) * 180 / math.pi


def margin(ang, mask):
    """the smallest distance of a valid, non-NaN angle to a threshold"""
    a = ang[mask[:, 0]]
    a = a[~torch.isnan(a)]
    return min(float((a - th).abs().min()) for th in THRESHOLDS) if a.numel() else math.inf


def call(ref, task, pred, target, mask):
    with np.errstate(all="ignore"):
        got = ref.get_metrics(pred, target, task=task, masks=mask.expand(-1, pred.shape[1], -1, -1))
    return None if got is None else {k: float(v) for k, v in got.items()}


def save(name, ref, task, pred, target, mask):
    pred, target = pred.float().contiguous(), target.float().contiguous()
    B = pred.shape[0]
    batch = call(ref, task, pred, target, mask)
    assert batch is not None, name
    keys = sorted(batch)
    images = np.full((B, len(keys)), np.nan)
    for i in range(B):
        one = call(ref, task, pred[i:i + 1], target[i:i + 1], mask[i:i + 1])
        assert (one is None) == (int(mask[i].sum()) == 0), (name, i)
        if one is not None:
            images[i] = [one[k] for k in keys]
    d = dict(task=np.array(task), pred=pred.numpy(), target=target.numpy(), mask=mask.numpy(), keys=np.array(keys),
             batch=np.array([batch[k] for k in keys], dtype=np.float64), images=images,
             num_valid=mask.reshape(B, -1).sum(1).numpy().astype(np.int64))
    note = ""
    if task == "normal":
        ang = angles(pred, target)
        mg = margin(ang, mask)
        assert mg >= MARGIN, (name, mg)
        valid = ang[mask[:, 0]]
        if not torch.isnan(valid).any():   # the stored angles are the reference's: its own mean and median of them
            assert abs(float(valid.mean()) - batch["ang_error_mean"]) <= 1e-12 * batch["ang_error_mean"], name
            assert float(np.median(valid.numpy())) == batch["ang_error_median"], name
        d["angles"] = ang.numpy()
        note = f", threshold margin {mg:.2e} deg, {len(np.unique(valid.numpy()))} distinct of {valid.numel()} valid angles"
    path = os.path.join(OUT, f"evalgpu_{name}.npz")
    np.savez_compressed(path, **d)
    print(f"{name}: num_valid {d['num_valid'].tolist()}{note}, {os.path.getsize(path)} B")
    print("   batch", {k: round(batch[k], 6) for k in keys})


def normal_case(seed, B, H, W, keep=0.75, noise=0.35):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(B, 3, H, W, generator=g)
    t = t / t.norm(dim=1, keepdim=True)
    p = t + noise * torch.randn(B, 3, H, W, generator=g)
    m = torch.rand(B, 1, H, W, generator=g) < keep
    return p * 0.5 + 0.5, t * 0.5 + 0.5, m   # the [0, 1] encoding the models output


def depth_case(seed, B, H, W, keep=0.75):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(B, 1, H, W, generator=g) * 0.9 + 0.05
    p = (t + 0.05 * torch.randn(B, 1, H, W, generator=g)).clamp(min=0.0)
    m = torch.rand(B, 1, H, W, generator=g) < keep
    return p, t, m


def set_parity(m, image, odd):
    """drops one valid pixel of the image where its count has the other parity"""
    if (int(m[image].sum()) % 2 == 1) != odd:
        idx = m[image].flatten().nonzero()[0, 0]
        m[image].view(-1)[idx] = False


def odd_masks(m):
    set_parity(m, 0, True)      # an odd count: the median is one element
    set_parity(m, 1, False)     # an even count: the mean of two
    m[2] = False                # an empty image


def first_seed(make, start):
    """the first seed from `start` whose case keeps the threshold margin"""
    for seed in range(start, start + 1000):
        p, t, m = make(seed)
        if margin(angles(p.float(), t.float()), m) >= MARGIN:
            return seed, p, t, m
    raise AssertionError("no seed with the threshold margin")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--omnidata", required=True, help="checkout of the reference repository")
    args = ap.parse_args()
    ref = load_reference(args.omnidata)
    torch.set_num_threads(4)

    # 1. an odd shape; image 0 with an odd count, image 1 with an even one, image 2 empty
    def odd(seed):
        p, t, m = normal_case(seed, 3, 37, 53)
        odd_masks(m)
        return p, t, m
    seed, p, t, m = first_seed(odd, 100)
    print("normal_odd: seed", seed)
    save("normal_odd", ref, "normal", p, t, m)
    p, t, m = depth_case(200, 3, 37, 53)
    odd_masks(m)
    save("depth_odd", ref, "depth_zbuffer", p, t, m)

    # 2. one valid pixel and two valid pixels: the median is the mean
    def few(seed):
        p, t, _ = normal_case(seed, 2, 5, 7)
        m = torch.zeros(2, 1, 5, 7, dtype=torch.bool)
        m[0, 0, 2, 3] = True
        m[1, 0, 0, 6] = True
        m[1, 0, 4, 1] = True
        return p, t, m
    seed, p, t, m = first_seed(few, 300)
    print("normal_few: seed", seed)
    save("normal_few", ref, "normal", p, t, m)

    # 3. ties: vectors of small integers give few distinct angles, many of them equal, some exactly on a threshold
    g = torch.Generator().manual_seed(400)
    p = torch.randint(-2, 3, (2, 3, 16, 20), generator=g).float()
    t = torch.randint(-2, 3, (2, 3, 16, 20), generator=g).float()
    m = torch.rand(2, 1, 16, 20, generator=g) < 0.9
    ang = angles(p, t)
    near = torch.zeros_like(m[:, 0])
    for th in THRESHOLDS:
        near |= (ang - th).abs() < MARGIN
    print(f"normal_ties: {int((near & m[:, 0]).sum())} valid pixels within {MARGIN} deg of a threshold masked out")
    m[:, 0] &= ~near
    save("normal_ties", ref, "normal", p, t, m)

    # 4. one NaN prediction inside the mask: np.median answers NaN, the thresholds compare false
    seed, p, t, m = first_seed(lambda s: normal_case(s, 2, 12, 16), 500)
    p[1, 1, 5, 7] = float("nan")
    m[1, 0, 5, 7] = True
    print("normal_nan: seed", seed)
    save("normal_nan", ref, "normal", p, t, m)

    # 5. depth with target == 0 at a masked-out pixel: (diff / target) * mask = NaN * 0 poisons rel_error alone
    p, t, m = depth_case(600, 2, 12, 16)
    t[0, 0, 3, 4] = 0.0
    p[0, 0, 3, 4] = 0.0
    m[0, 0, 3, 4] = False
    save("depth_zero_target", ref, "depth_zbuffer", p, t, m)


if __name__ == "__main__":
    main()
