"""The cases of the blur chain that tests/test_gpu_augment.py (on the GPU) and tests/test_augment_cpu_build.py (the host build)
share, and their bar: max |got - r64| <= 2 max |r32 - r64| + 2e-6 with r32, r64 the restatement in the two precisions."""
import itertools

import numpy as np
import torch

import augment_restatement as R
from omnidata_amd import augmentation as A

B = 3
# 2x5: sharpness is the identity; 3x3: one interior pixel; 7x9: smaller than any tile, every reflect legal; 17x65, 33x130, 64x128:
# partial tiles, several tiles, whole tiles; 33x65: one pixel more than the kernel's 32 x 64 output tile in each axis
SHAPES = ((2, 5), (3, 3), (7, 9), (17, 65), (33, 130), (64, 128), (33, 65))
COMBOS = ("s", "m", "g", "sm", "sg", "mg", "smg")
MOTION_SIZES = (3, 5, 7)
GAUSS_SIZES = ((1, 7), (5, 3), (7, 7), (3, 5), (7, 1), (3, 3), (5, 5), (1, 1))


def cases():
    """(H, W, C, combo, km, (ky, kx)): every shape x C in {1, 3} x every combination of stages; the filter sizes rotate so that
    every size meets every kind of shape, cut to what the reflect border allows (H > ky // 2, W > kx // 2)."""
    out = []
    n = itertools.count()
    for (H, W), C, combo in itertools.product(SHAPES, (1, 3), COMBOS):
        i = next(n)
        km = MOTION_SIZES[i % 3]
        ky, kx = GAUSS_SIZES[(i // 2) % len(GAUSS_SIZES)]
        ky, kx = min(ky, 2 * H - 1), min(kx, 2 * W - 1)
        out.append((H, W, C, combo, km, (ky, kx)))
    return out


def case_id(c):
    return f"{c[0]}x{c[1]}-C{c[2]}-{c[3]}-m{c[4]}-g{c[5][0]}x{c[5][1]}"


def image(C, H, W, seed=0, batch=B):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.rand(batch, C, H, W, generator=g)


def parameters(combo, km, gsize, seed=0, batch=B):
    """{'sharpness', 'motion', 'gaussian'} as filter_chain takes them, different for every sample"""
    g = torch.Generator().manual_seed(2000 + seed)
    u = lambda: torch.rand(batch, generator=g).double()
    p = {"sharpness": None, "motion": None, "gaussian": None}
    if "s" in combo:
        f = (u() * 0.9).tolist()
        f[-1] = 1.0 if seed % 2 else 0.0                      # the two ends of the blend
        p["sharpness"] = f
    if "m" in combo:
        p["motion"] = (km, ((2 * u() - 1) * 50.0).tolist(), (2 * u() - 1).tolist())
    if "g" in combo:
        sy, sx = (0.1 + 1.9 * u()).tolist(), (0.1 + 1.9 * u()).tolist()
        p["gaussian"] = (gsize, list(zip(sy, sx)))
    return p


def restated(x, plan, dtype):
    t = lambda a: None if a is None else torch.from_numpy(a)
    return R.chain(x, t(plan.sharp), t(plan.motion), None if plan.gy is None else (t(plan.gy), t(plan.gx)), dtype)


def judge(got, x, plan, what):
    """the bar; returns (err, E)"""
    r64, r32 = restated(x, plan, torch.float64), restated(x, plan, torch.float32)
    E = float((r32.double() - r64).abs().max())
    err = float((got.double().cpu() - r64).abs().max())
    print(f"[augment] {what}: E {E:.3e} err {err:.3e} err / (2 E + 2e-6) {err / (2 * E + 2e-6):.3f}")
    assert err <= 2 * E + 2e-6, what
    return err, E


def plan_of(case, seed=0, batch=B):
    H, W, C, combo, km, gsize = case
    return A.plan_filter_chain(batch, **parameters(combo, km, gsize, seed, batch))
