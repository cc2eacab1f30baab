"""The training augmentations on the GPU (omnidata_amd/augmentation.py over csrc/augment.hip): the blur chain against the restatement
in fp64 at the project's bar (tests/augment_cases.py), planted cases that a bound cannot hide, the structural guarantees of the
header, resize_tasks against CPU ATen and the reference's recorded outputs, and Augmentation against its own plan."""
import json
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_cases as cases
import augment_restatement as R
from gpu_util import f32_guards_intact, guarded_f32
from omnidata_amd import augmentation as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TASKS = ("rgb", "depth_zbuffer", "mask_valid")


# ------------------------------------------------------------------------------------------------ the chain against the bar
@pytest.mark.parametrize("case", cases.cases(), ids=cases.case_id)
def test_chain_is_within_the_bar_of_the_restatement(case):
    H, W, C = case[:3]
    x = cases.image(C, H, W)
    p = cases.parameters(case[3], case[4], case[5])
    got = A.filter_chain(x.to(DEV), **p)
    cases.judge(got, x, cases.plan_of(case), cases.case_id(case))


# ------------------------------------------------------------------------------------------------ planted cases
@pytest.mark.parametrize("k", [3, 5, 7])
def test_a_delta_returns_each_samples_own_motion_taps_mirrored(k):
    H, W, cy, cx = 11, 13, 5, 7
    x = torch.zeros(3, 2, H, W)
    x[:, :, cy, cx] = 1.0
    angle, direction = [30.0, -45.0, 10.0], [0.8, -0.6, 0.3]
    plan = A.plan_filter_chain(3, motion=(k, angle, direction))
    got = A.motion_blur(x.to(DEV), k, angle, direction).cpu()
    m = k // 2
    for b in range(3):
        taps = torch.from_numpy(plan.motion[b])
        assert not torch.equal(taps, taps.flip(0, 1)) and not torch.equal(taps, torch.from_numpy(plan.motion[(b + 1) % 3]))
        want = torch.zeros(H, W)
        want[cy - m:cy + m + 1, cx - m:cx + m + 1] = taps.flip(0, 1)     # out(y, x) = t[cy - y + m][cx - x + m]
        for c in range(2):
            assert torch.equal(got[b, c], want), (b, c)


def test_ones_under_motion_blur_give_the_partial_tap_sums_in_the_corners():
    k, H, W = 7, 9, 70
    angle, direction = [40.0, -20.0, 0.0], [1.0, -0.3, 0.5]
    plan = A.plan_filter_chain(3, motion=(k, angle, direction))
    got = A.motion_blur(torch.ones(3, 1, H, W, device=DEV), k, angle, direction).cpu().double()
    t = torch.from_numpy(plan.motion).double()
    m = k // 2
    for b in range(3):
        corners = {(0, 0): t[b, m:, m:], (0, W - 1): t[b, m:, :m + 1], (H - 1, 0): t[b, :m + 1, m:], (H - 1, W - 1): t[b, :m + 1, :m + 1]}
        for (y, x), part in corners.items():
            assert abs(float(got[b, 0, y, x]) - float(part.sum())) <= 1e-6, (b, y, x)
        assert abs(float(got[b, 0, H // 2, W // 2]) - 1.0) <= 1e-6
    assert len({round(float(got[b, 0, 0, 0]), 5) for b in range(3)}) == 3


def test_a_ramp_under_the_gaussian_stays_a_ramp_inside_and_folds_at_the_border():
    H, W = 40, 70
    gy, gx = A.gaussian_table(5, 1.3), A.gaussian_table(3, 0.8)
    col = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W).expand(1, 1, H, W) / 64.0
    row = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1).expand(1, 1, H, W) / 64.0
    got = A.gaussian_blur(torch.cat([col, row]).to(DEV), (5, 3), [(1.3, 0.8)] * 2).cpu().double()
    assert float((got[0, 0, :, 1:-1] - col[0, 0, :, 1:-1].double()).abs().max()) <= 1e-6          # inside: the ramp itself
    assert float((got[1, 0, 2:-2] - row[0, 0, 2:-2].double()).abs().max()) <= 1e-6
    fold = gx[0] + gx[2]                                                                          # columns -1 -> 1 and W -> W - 2
    assert float((got[0, 0, :, 0] - fold / 64.0).abs().max()) <= 1e-6
    assert float((got[0, 0, :, -1] - (W - 1 - fold) / 64.0).abs().max()) <= 1e-6
    top0 = 2 * gy[0] * 2 + 2 * gy[1] * 1                                                          # rows 2 1 0 1 2
    top1 = gy[0] * 1 + gy[1] * 0 + gy[2] * 1 + gy[3] * 2 + gy[4] * 3                              # rows 1 0 1 2 3
    assert float((got[1, 0, 0] - top0 / 64.0).abs().max()) <= 1e-6 and float((got[1, 0, 1] - top1 / 64.0).abs().max()) <= 1e-6
    assert float((got[1, 0, -1] - (H - 1 - top0) / 64.0).abs().max()) <= 1e-6


# ------------------------------------------------------------------------------------------------ structure
ALL = dict(sharpness=[0.1, 0.5, 0.9], motion=(7, [12.0, -33.0, 48.0], [0.2, -0.9, 0.6]), gaussian=((5, 7), [0.7, (0.3, 1.9), 1.4]))


def test_canaries_two_runs_batch_independence_and_views():
    x = cases.image(3, 33, 65, seed=4).to(DEV)
    buf, payload = guarded_f32(x.numel(), 4096)
    out = A.filter_chain(x, **ALL, out=payload.view(x.shape))
    torch.cuda.synchronize()
    assert f32_guards_intact(buf, x.numel(), 4096) and not bool(torch.isnan(out).any())
    again = A.filter_chain(x, **ALL)
    assert torch.equal(out, again)                                                                # two runs, the same bits
    alone = A.filter_chain(x[1:2].clone(), sharpness=ALL["sharpness"][1], motion=(7, ALL["motion"][1][1], ALL["motion"][2][1]),
                           gaussian=((5, 7), [ALL["gaussian"][1][1]]))
    assert torch.equal(alone[0], out[1])                                                          # image 1 of 3 = the image alone
    wide = torch.rand(3, 3, 33, 130, device=DEV)
    view = wide[:, :, :, ::2]
    assert not view.is_contiguous()
    assert torch.equal(A.filter_chain(view, **ALL), A.filter_chain(view.contiguous(), **ALL))
    cl = x.contiguous(memory_format=torch.channels_last)
    assert torch.equal(A.filter_chain(cl, **ALL), out)
    # every stage alone is what the one-stage wrappers give, and a sample with factor 1 passes through sharpness bit for bit
    assert torch.equal(A.sharpness(x, [0.3, 1.0, 0.0])[1], x[1])
    assert torch.equal(A.sharpness(x, 0.25), A.filter_chain(x, sharpness=0.25))
    assert torch.equal(A.filter_chain(x), x) and A.filter_chain(x).data_ptr() != x.data_ptr()


def test_what_raises():
    x = cases.image(1, 3, 9).to(DEV)
    with pytest.raises(ValueError, match="alias"):
        A.filter_chain(x, sharpness=0.5, out=x)
    with pytest.raises(ValueError, match="device tensor"):
        A.filter_chain(x, sharpness=torch.full((3,), 0.5, device=DEV))
    with pytest.raises(ValueError, match="reflect"):
        A.gaussian_blur(x, (7, 3), 1.0)                                                           # H = 3 <= 7 // 2
    with pytest.raises(ValueError):
        A.filter_chain(x.cpu(), sharpness=0.5)
    with pytest.raises(ValueError):
        A.filter_chain(x.double(), sharpness=0.5)
    d = torch.rand(2, 1, 20, 24, device=DEV)
    with pytest.raises(ValueError, match="does not fit"):
        A.resize_tasks({"d": d}, ["d"], "crop", (16, 16), (5, 0))
    with pytest.raises(ValueError):
        A.resize_tasks({"rgb": d.to(torch.uint8)}, ["rgb"], "resize", (16, 16))                   # bilinear needs float32
    with pytest.raises(ValueError):
        A.resize_tasks({"d": d, "e": d[:, :, :10]}, ["d", "e"], "resize", (16, 16))


def test_chain_under_a_captured_graph_replays_to_the_same_bits():
    x = cases.image(3, 33, 130, seed=9).to(DEV)
    tables = A.upload(A.plan_filter_chain(3, **ALL), DEV)                                          # the upload stays outside the graph
    out = torch.empty_like(x)
    A.filter_chain(x, tables=tables, out=out)
    torch.cuda.synchronize()
    want = out.clone()
    assert torch.equal(want, A.filter_chain(x, **ALL))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        A.filter_chain(x, tables=tables, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


# ------------------------------------------------------------------------------------------------ resize_tasks
def _batch(src, seed=5):
    g = torch.Generator().manual_seed(seed)
    return {"rgb": torch.rand(2, 3, *src, generator=g), "depth_zbuffer": torch.rand(2, 1, *src, generator=g),
            "mask_valid": torch.rand(2, 1, *src, generator=g) < 0.5, "semantic": torch.randint(0, 256, (2, 1, *src), generator=g).to(torch.uint8)}


@pytest.mark.parametrize("src,dst", [((72, 80), (48, 48)), ((80, 72), (64, 48)), ((37, 53), (53, 37))])
def test_resize_tasks_against_cpu_aten_and_slicing(src, dst):
    cpu = _batch(src)
    names = list(cpu)
    dev = {k: v.to(DEV) for k, v in cpu.items()}
    h, w = dst
    got = A.resize_tasks(dev, names, "resize", dst)                                               # four tasks, one launch
    for k in names[1:]:
        want = F.interpolate(cpu[k].float(), dst, mode="nearest").to(cpu[k].dtype)
        assert got[k].dtype == cpu[k].dtype and torch.equal(got[k].cpu(), want), k
        assert torch.equal(got[k].cpu(), R.resize_nearest(cpu[k], h, w))
    r64 = F.interpolate(cpu["rgb"].double(), dst, mode="bilinear", align_corners=False)
    E = float((R.resize_bilinear(cpu["rgb"], h, w).double() - r64).abs().max())
    err = float((got["rgb"].cpu().double() - r64).abs().max())
    print(f"[augment] bilinear {src} -> {dst}: E {E:.3e} err {err:.3e} err / (2 E + 2e-6) {err / (2 * E + 2e-6):.3f}")
    assert err <= 2 * E + 2e-6
    for k in names:                                                                               # against four separate calls
        assert torch.equal(A.resize_tasks(dev, [k], "resize", dst)[k], got[k]), k
    if h <= src[0] and w <= src[1]:
        y0, x0 = src[0] - h, (src[1] - w) // 2
        crop = A.resize_tasks(dev, names, "randomcrop", dst, (y0, x0))
        for k in names:
            assert crop[k].dtype == cpu[k].dtype and torch.equal(crop[k].cpu(), cpu[k][:, :, y0:y0 + h, x0:x0 + w]), k
            assert torch.equal(A.resize_tasks(dev, [k], "crop", dst, (y0, x0))[k], crop[k])
        centre = A.resize_tasks(dev, names, "centercrop", dst)
        cy, cx = (src[0] - h) // 2, (src[1] - w) // 2
        assert torch.equal(centre["rgb"].cpu(), cpu["rgb"][:, :, cy:cy + h, cx:cx + w])
    views = {k: v.transpose(2, 3).contiguous().transpose(2, 3) for k, v in dev.items()}           # non-contiguous sources
    assert all(torch.equal(A.resize_tasks(views, names, "resize", dst)[k], got[k]) for k in names)


def test_resize_tasks_and_resize_augmentation_against_the_golden_files():
    d = np.load(os.path.join(GOLDEN, "augment_resize_decisions.npz"))
    recs = json.loads(str(d["small"]))
    inputs = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "augment_resize_small_inputs.npz")).items()}
    outputs = {}
    for k in range(4):
        outputs.update(np.load(os.path.join(GOLDEN, f"augment_resize_small_outputs_{k}.npz")).items())
    aug = A.Augmentation()
    done = set()
    for rec in recs:
        if not rec["completed"]:
            continue
        random.seed(rec["seed"])
        batch = aug.resize_augmentation({k: v.to(DEV) for k, v in inputs.items()}, list(TASKS), fixed_size=48)
        want = {t: torch.from_numpy(outputs[f"s{rec['output_seed']}_{t}"]) for t in TASKS}
        for t in TASKS:
            if rec["method"] == "resize" and t == "rgb":   # CPU ATen's own roundings: tests/test_augment_host.py bounds the definition's
                # distance from them by 2 x 2^-18 + 4 x 2^-24; the kernel's own four roundings come on top
                assert float((batch[t].cpu() - want[t]).abs().max()) <= 2 * 2.0 ** -18 + 8 * 2.0 ** -24
            else:
                assert torch.equal(batch[t].cpu(), want[t]), (rec["seed"], t)
        done.add(rec["method"])
    assert done == {"randomcrop", "resize"}


# ------------------------------------------------------------------------------------------------ Augmentation
def test_augmentation_equals_the_kernels_called_with_its_plan():
    rgb = cases.image(3, 40, 72, seed=11).to(DEV)
    depth = torch.rand(3, 1, 40, 72, device=DEV) * 1.5
    aug = A.Augmentation()
    ran = 0
    for seed in range(12):
        random.seed(seed)
        got = aug.augment_rgb({"positive": {"rgb": rgb}}, generator=torch.Generator().manual_seed(100 + seed))
        random.seed(seed)
        plan = A.plan_rgb(3, torch.Generator().manual_seed(100 + seed))
        if plan["sharpness"] is None and plan["motion"] is None and plan["gaussian"] is None:
            assert got is rgb
            continue
        assert torch.equal(got, A.filter_chain(rgb, plan["sharpness"], plan["motion"], plan["gaussian"]))
        ran += 1
    assert ran >= 5
    for seed in range(6):
        random.seed(seed)
        plan = A.plan_resize((40, 72), 32)
        random.seed(seed)
        batch = aug.resize_augmentation({"rgb": rgb.clone(), "depth_zbuffer": depth[0].clone()}, ["rgb"], fixed_size=32)
        assert torch.equal(batch["rgb"], A.resize_tasks({"rgb": rgb}, ["rgb"], plan["method"], plan["size"], plan["offset"])["rgb"])
    random.seed(0)
    batch = aug.resize_augmentation({"depth_zbuffer": depth[0].clone()}, ["depth_zbuffer"], fixed_size=32)
    assert batch["depth_zbuffer"].shape == (1, 1, 32, 32)                                         # a 3-D tensor gets its batch axis


def test_augmentation_refocus_slot_runs_the_refocus_module_behind_the_chain():
    from omnidata_amd.refocus import RefocusImageAugmentation
    seed = next(s for s in range(200) if (random.seed(s), A.plan_rgb(2, torch.Generator().manual_seed(s), refocus=True))[1]["refocus"])
    rgb = cases.image(3, 32, 48, seed=12, batch=2).to(DEV)
    depth = (0.2 + 1.2 * torch.rand(2, 1, 32, 48, generator=torch.Generator().manual_seed(1))).to(DEV)     # some of it >= 1
    before = depth.clone()
    refocus = RefocusImageAugmentation(10, 0.005, 6.0)
    aug = A.Augmentation(refocus=refocus)
    random.seed(seed)
    torch.manual_seed(7)
    got = aug.augment_rgb({"positive": {"rgb": rgb, "depth_euclidean": depth}}, generator=torch.Generator().manual_seed(seed))
    assert torch.equal(depth, before)                                                             # the caller's depth is left alone
    random.seed(seed)
    plan = A.plan_rgb(2, torch.Generator().manual_seed(seed), refocus=True)
    mid = rgb if plan["sharpness"] is None and plan["motion"] is None else A.filter_chain(rgb, plan["sharpness"], plan["motion"])
    assert plan["gaussian"] is None
    d = depth.clone()
    d[d >= 1.0] = d[d < 1.0].max()
    torch.manual_seed(7)
    assert torch.equal(got, refocus(mid, d))
    random.seed(seed)
    assert not A.plan_rgb(2, torch.Generator().manual_seed(seed))["refocus"]                      # off by default
