"""The host side of the training augmentations (omnidata_amd/augmentation.py) and their restatement (tests/augment_restatement.py),
without a GPU: the decisions of resize_augmentation and augment_rgb against the reference's, recorded call by call for
random.seed(0..31) (tests/golden/augment_resize_*.npz, tools/make_augment_golden.py); the restatement's crop / nearest / bilinear
against the reference's outputs; the tap tables against their known shapes and formulas; sharpness against Pillow."""
import json
import os
import random

import numpy as np
import pytest
import torch

import augment_restatement as R
from omnidata_amd import augmentation as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TASKS = ("rgb", "depth_zbuffer", "mask_valid")


@pytest.fixture(scope="module")
def decisions():
    d = np.load(os.path.join(GOLDEN, "augment_resize_decisions.npz"))
    return {k: json.loads(str(d[k])) for k in ("small", "free512", "rgb")}


@pytest.fixture(scope="module")
def small():
    inputs = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "augment_resize_small_inputs.npz")).items()}
    outputs = {}
    for k in range(4):
        outputs.update(np.load(os.path.join(GOLDEN, f"augment_resize_small_outputs_{k}.npz")).items())
    return inputs, {k: torch.from_numpy(v) for k, v in outputs.items()}


class Recorder:
    """the `random` module with every call recorded as [name, args, result], as tools/make_augment_golden.py records them"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        f = getattr(random, name)

        def wrapped(*args):
            r = f(*args)
            self.calls.append([name, list(args), r])
            return r
        return wrapped


def recorded(monkeypatch, seed, fn):
    rec = Recorder()
    monkeypatch.setattr(A, "random", rec)
    random.seed(seed)
    try:
        result, error = fn(), None
    except Exception as e:
        result, error = None, e
    return json.loads(json.dumps(rec.calls)), result, error


@pytest.mark.parametrize("mode,src,fixed", [("small", (72, 80), 48), ("free512", (512, 512), None)])
def test_resize_decisions_equal_the_references_seed_for_seed(decisions, monkeypatch, mode, src, fixed):
    assert [r["seed"] for r in decisions[mode]] == list(range(32))
    assert [r["seed"] for r in decisions[mode] if r["completed"]][:7] == [0, 2, 5, 6, 9, 10, 11]
    methods = set()
    for want in decisions[mode]:
        calls, plan, error = recorded(monkeypatch, want["seed"], lambda: A.plan_resize(src, fixed))
        assert calls == want["calls"], want["seed"]                       # the same calls, arguments and results, in order
        assert error is None
        assert plan["method"] == want["method"] and list(plan["size"]) == want["size"], want["seed"]
        methods.add(plan["method"])
        if plan["method"] == "randomcrop":
            assert list(plan["offset"]) == want["offset"], want["seed"]   # (min_x, min_y): the row and the column offset
        elif plan["method"] == "centercrop":                              # the reference stops at kornia's CenterCrop, after its draws
            assert not want["completed"] and "CenterCrop" in want["error"]
            assert plan["offset"] == ((src[0] - plan["size"][0]) // 2, (src[1] - plan["size"][1]) // 2)
        else:
            assert plan["offset"] is None and want["completed"]
    assert methods == {"centercrop", "randomcrop", "resize"}


def test_an_empty_randrange_raises_as_in_the_reference_and_a_centred_window_must_fit(monkeypatch):
    seeds = {}
    for s in range(32):
        random.seed(s)
        p = random.random()
        seeds.setdefault("centercrop" if p < 0.4 else "randomcrop" if p < 0.7 else "resize", s)
    random.seed(seeds["randomcrop"])
    with pytest.raises(ValueError):
        A.plan_resize((49, 80), 48)                                       # randrange(0, 49 - 48 - 2)
    random.seed(seeds["randomcrop"])
    assert A.plan_resize((48, 48), 48)["offset"] == (0, 0)                # equal sizes: no draw
    random.seed(seeds["centercrop"])
    with pytest.raises(ValueError, match="does not fit"):
        A.plan_resize((40, 80), 48)


def test_rgb_decisions_equal_the_references_seed_for_seed(decisions, monkeypatch):
    seen = set()
    for want in decisions["rgb"]:
        assert want["error"] is None
        gen = torch.Generator().manual_seed(want["seed"])
        calls, plan, error = recorded(monkeypatch, want["seed"], lambda: A.plan_rgb(2, gen))
        assert error is None and calls == want["calls"], want["seed"]
        made = {m[0]: m[1] for m in want["made"]}
        assert [m[0] for m in want["made"]] == [n for n in ("RandomSharpness", "RandomMotionBlur", "RandomGaussianBlur") if n in made]
        assert (plan["sharpness"] is not None) == ("RandomSharpness" in made)
        assert (plan["motion"] is not None) == ("RandomMotionBlur" in made)
        assert (plan["gaussian"] is not None) == ("RandomGaussianBlur" in made)
        if plan["sharpness"] is not None:
            assert made["RandomSharpness"] == [0.3] and all(0.0 <= f <= 0.3 for f in plan["sharpness"])
        if plan["motion"] is not None:
            assert made["RandomMotionBlur"] == [[3, 7], plan["motion_amount"], 0.5]
            k, angle, direction = plan["motion"]
            assert k in (3, 5, 7) and all(abs(a) <= plan["motion_amount"] for a in angle) and all(abs(d) <= 0.5 for d in direction)
        if plan["gaussian"] is not None:
            k = plan["gaussian_size"]
            assert made["RandomGaussianBlur"] == [[k, k], [0.1, 2.0]] and plan["gaussian"][0] == k
            assert all(0.1 <= s <= 2.0 for s in plan["gaussian"][1])
        seen.add((plan["sharpness"] is not None, plan["motion"] is not None, plan["gaussian_size"]))
    assert len(seen) >= 6                                                  # the seeds reach most branches


def test_rgb_parameters_come_from_the_generator_in_stage_order_and_only_for_active_stages(monkeypatch):
    for seed in range(32):
        gen, twin = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
        random.seed(seed)
        plan = A.plan_rgb(3, gen)
        u = lambda n: torch.rand(n, generator=twin).double()
        if plan["sharpness"] is not None:
            assert plan["sharpness"] == (u(3) * 0.3).tolist()
        if plan["motion"] is not None:
            assert plan["motion"][0] == 3 + 2 * min(int(float(u(1)) * 3.0), 2)
            assert plan["motion"][1] == ((2.0 * u(3) - 1.0) * plan["motion_amount"]).tolist()
            assert plan["motion"][2] == ((2.0 * u(3) - 1.0) * 0.5).tolist()
        if plan["gaussian"] is not None:
            assert plan["gaussian"][1] == (0.1 + u(3) * 1.9).tolist()
        assert torch.equal(gen.get_state(), twin.get_state())              # nothing else was drawn
        random.seed(seed)
        pair = A.plan_rgb(3, torch.Generator().manual_seed(seed), gaussian_sigma="pair")
        if pair["gaussian"] is not None:
            assert pair["gaussian"][1] == [(0.1, 2.0)] * 3


def _golden_cases(decisions, small, method):
    inputs, outputs = small
    for rec in decisions["small"]:
        if rec["completed"] and rec["method"] == method:
            yield rec, inputs, {t: outputs[f"s{rec['output_seed']}_{t}"] for t in TASKS}


def test_restatement_crop_and_nearest_equal_the_golden_outputs_bit_for_bit(decisions, small):
    n = 0
    for rec, inputs, want in _golden_cases(decisions, small, "randomcrop"):
        for t in TASKS:
            assert torch.equal(R.crop(inputs[t], *rec["offset"], *rec["size"]), want[t]), (rec["seed"], t)
        n += 1
    for rec, inputs, want in _golden_cases(decisions, small, "resize"):
        for t in TASKS[1:]:
            assert torch.equal(R.resize_nearest(inputs[t], *rec["size"]), want[t]), (rec["seed"], t)
        n += 1
    assert n >= 10
    for src, dst in ((512, 256), (512, 320), (512, 384), (512, 448), (72, 48), (80, 48), (37, 53)):   # the index rule itself
        x = torch.arange(src, dtype=torch.float32).view(1, 1, 1, src)
        assert torch.equal(R.nearest_index(src, dst).float(), torch.nn.functional.interpolate(x, (1, dst), mode="nearest")[0, 0, 0])


def test_restatement_bilinear_is_within_the_coordinate_rounding_of_the_golden_outputs(decisions, small):
    """The golden rgb outputs are CPU ATen's.  Its build forms the source coordinate with one fused multiply-subtract,
    fma(scale, dst + 0.5, -0.5), where the definition (and fullframe.hip, whose arithmetic the kernel shares) rounds the product
    first: the coordinates differ by at most half an ulp of the product, 2^-18 for sources below 128 pixels, on either axis, and
    the blend of values in [0, 1] moves by at most that; the blend's own roundings add 4 x 2^-24."""
    n = 0
    for rec, inputs, want in _golden_cases(decisions, small, "resize"):
        got = R.resize_bilinear(inputs["rgb"], *rec["size"])
        err = float((got - want["rgb"]).abs().max())
        print(f"seed {rec['seed']}: max |restatement - golden| {err:.3e}")
        assert err <= 2 * 2.0 ** -18 + 4 * 2.0 ** -24
        n += 1
    assert n >= 4
    x = torch.rand(2, 3, 37, 53, generator=torch.Generator().manual_seed(3))          # a size whose coordinates are not exact either way
    for h, w in ((53, 37), (64, 48)):
        err = float((R.resize_bilinear(x, h, w) - torch.nn.functional.interpolate(x, (h, w), mode="bilinear")).abs().max())
        assert err <= 2 * 2.0 ** -18 + 4 * 2.0 ** -24


def test_restatement_bilinear_equals_the_golden_outputs_bit_for_bit(decisions, small):
    """The golden rgb outputs are CPU ATen's, and ATen's compiled arithmetic is not the definition's (resize_bilinear: the
    arithmetic of dptx_postprocess_resize_batch, which the kernel keeps): with the definition 23.1 % of the elements of
    72 x 80 -> 48 x 48 are one ulp (1.19e-7) off.  The restatement therefore also states ATen's own arithmetic for such tensors
    (resize_bilinear_aten_cpu: a fused coordinate, four product weights, one product and three fmas in the order b, a, c, d),
    recovered from ATen's results alone, and THAT equals the recorded outputs bit for bit; the test above bounds the distance
    between the two."""
    n = 0
    for rec, inputs, want in _golden_cases(decisions, small, "resize"):
        got = R.resize_bilinear_aten_cpu(inputs["rgb"], *rec["size"])
        assert got.dtype == torch.float32 and torch.equal(got, want["rgb"]), (rec["seed"], float((got - want["rgb"]).abs().max()))
        for t in TASKS[1:]:                                               # the model is not a copy of the file: it differs from nearest
            assert not torch.equal(R.resize_bilinear_aten_cpu(inputs[t], *rec["size"]), want[t])
        n += 1
    assert n >= 4
    # the model against the definition: the same weights up to the fused coordinate, so no further apart than the bound above
    x = inputs["rgb"]
    assert float((R.resize_bilinear_aten_cpu(x, 48, 48) - R.resize_bilinear(x, 48, 48)).abs().max()) <= 2 * 2.0 ** -18 + 4 * 2.0 ** -24


def test_motion_tables_known_shapes_sum_and_direction():
    t = A.motion_table(5, 0.0, 0.5)
    want = np.zeros((5, 5))
    want[2] = [.3, .25, .2, .15, .1]
    assert np.allclose(t, want, atol=1e-15)
    t = A.motion_table(5, 45.0, 0.0)
    want = np.zeros((5, 5))
    want[1, 3] = want[2, 2] = want[3, 1] = 1.0 / 3.0                      # anti-diagonal: anti-clockwise with y down
    assert np.allclose(t, want, atol=1e-15)
    t = A.motion_table(3, 90.0, -0.5)
    want = np.zeros((3, 3))
    want[:, 1] = [.5, 1.0 / 3.0, 1.0 / 6.0]
    assert np.allclose(t, want, atol=1e-15)
    smallest = 9.0
    for k in (3, 5, 7):
        for angle in np.linspace(-50.0, 50.0, 201):
            for direction in (-1.0, -0.5, 0.0, 0.5, 1.0):
                t = A.motion_table(k, angle, direction)
                assert abs(t.sum() - 1.0) < 1e-14 and (t >= 0).all() and t.shape == (k, k)
                assert t[k // 2, k // 2] > 0                               # the centre tap is 0.5 before the division
                smallest = min(smallest, 0.5 / t[k // 2, k // 2])
        assert A.motion_table(k, 0.0, 1.0)[k // 2, -1] == 0 and (A.motion_table(k, 0.0, 1.0)[k // 2, :-1] > 0).all()
        assert A.motion_table(k, 0.0, -1.0)[k // 2, 0] == 0 and (A.motion_table(k, 0.0, -1.0)[k // 2, 1:] > 0).all()
        assert np.array_equal(A.motion_table(k, 0.0, 3.0), A.motion_table(k, 0.0, 1.0))               # direction is clamped
    assert abs(smallest - 1.5) < 1e-12                                    # the smallest sum before the division
    angles, directions = np.linspace(-50.0, 50.0, 33), np.linspace(-1.2, 1.2, 33)
    for k in (3, 5, 7):                                                   # a batch of tables is the tables one by one
        both = A.motion_tables(k, angles, directions)
        assert both.shape == (33, k, k)
        assert all(np.array_equal(both[i], A.motion_table(k, angles[i], directions[i])) for i in range(33))
    with pytest.raises(ValueError):
        A.motion_table(4, 0.0, 0.0)


def test_gaussian_tables_and_the_plan():
    for k in (1, 3, 5, 7):
        for sigma in (0.1, 0.5, 1.0, 2.0):
            g = A.gaussian_table(k, sigma)
            want = np.array([np.exp(-((i - k // 2) ** 2) / (2 * sigma * sigma)) for i in range(k)])
            assert np.allclose(g, want / want.sum(), rtol=1e-15, atol=0) and abs(g.sum() - 1) < 1e-15
    plan = A.plan_filter_chain(3, sharpness=0.25, motion=(5, [0.0, 10.0, -30.0], torch.tensor([0.0, 0.5, -0.5])),
                               gaussian=((1, 7), [0.5, (0.1, 2.0), 1.0]))
    assert plan.sharp.dtype == np.float32 and plan.sharp.tolist() == [0.25] * 3
    assert plan.motion.shape == (3, 5, 5) and plan.gy.shape == (3, 1) and plan.gx.shape == (3, 7)
    assert np.array_equal(plan.motion[1], A.motion_table(5, 10.0, 0.5).astype(np.float32))           # rounded once
    assert np.array_equal(plan.gx[1], A.gaussian_table(7, 2.0).astype(np.float32)) and (plan.gy == 1).all()
    with pytest.raises(ValueError):
        A.plan_filter_chain(3, sharpness=[0.1, 0.2])                      # two values for three samples
    with pytest.raises(ValueError):
        A.plan_filter_chain(3, sharpness=1.5)
    with pytest.raises(ValueError):
        A.plan_filter_chain(3, gaussian=(4, 1.0))
    assert not A.plan_filter_chain(3).active


def test_sharpness_restatement_against_pillow():
    """PIL rounds twice (the SMOOTH filter's result to uint8, then the blend): 1.32 levels measured before rounding on this case"""
    from PIL import Image, ImageEnhance
    rng = np.random.default_rng(7)
    px = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    img = Image.fromarray(px, "RGB")
    x = torch.from_numpy(px).permute(2, 0, 1).unsqueeze(0).float() / 255.0
    for f in (0.0, 0.1, 0.3, 0.7, 1.0):
        want = np.asarray(ImageEnhance.Sharpness(img).enhance(f)).astype(np.int64)
        got = (R.sharpness(x, f) * 255.0)[0].permute(1, 2, 0)
        raw = float((got.double() - torch.from_numpy(want)).abs().max())
        levels = int((got.round().long() - torch.from_numpy(want)).abs().max())
        print(f"sharpness f={f}: {raw:.2f} levels before rounding, {levels} after")
        assert levels <= 2
    assert torch.equal(R.sharpness(x, 1.0), x)                            # f == 1: x, bit for bit
    assert torch.equal(R.sharpness(x[:, :, :2], 0.0), x[:, :, :2])        # H < 3: no interior
