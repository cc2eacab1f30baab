"""Writes tests/golden/augment_resize_*.npz: the decisions and the outputs of the reference's training augmentations, run on the CPU.

    python tools/make_augment_golden.py --omnidata <checkout of EPFL-VILAB/omnidata>

Loads omnidata_tools/torch/data/augmentation.py from that checkout at run time (nothing of it is copied here), with the `seaborn`
stub of tools/make_refocus_golden.py.  The module's `random` is wrapped so that every call is recorded with its arguments and its
result; the method, the size and the offsets are read from the locals of the reference's own frame when it returns or raises.

resize_augmentation runs for `random.seed(0..31)` in two modes: a small source [2,C,72,80] with fixed_size=48 for the tasks rgb,
depth_zbuffer and a 0/1 mask_valid (inputs, decisions and the outputs of the seeds that complete), and a 512 x 512 source with
free sizes (decisions only).  Without kornia 'randomcrop' and 'resize' run and 'centercrop' raises NameError after its draws: such
a seed keeps its decisions and has no output.

augment_rgb needs kornia's classes by name even to start (ColorJitter is constructed first).  They are replaced by stand-ins that
record their constructor arguments and return their input, so that the reference's own code makes its draws: recorded per seed
are the `random` calls and the (class, arguments) list.  What kornia would have drawn inside those classes is not recorded.

    augment_resize_decisions.npz        JSON strings 'small', 'free512', 'rgb': one record per seed
    augment_resize_small_inputs.npz     rgb [2,3,72,80], depth_zbuffer [2,1,72,80], mask_valid [2,1,72,80], fp32 multiples of 1/256
    augment_resize_small_outputs_<k>.npz  's<seed>_<task>' for the seeds 8k .. 8k + 7 that complete; seeds with the same decisions
                                        share one output (the record's 'output_seed')
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
TASKS = ["rgb", "depth_zbuffer", "mask_valid"]
SEEDS = range(32)
LIMIT = 300 * 1000


class RecordingRandom:
    """the `random` module with every call recorded as [name, args, result]"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        f = getattr(random, name)
        if not callable(f):
            return f

        def wrapped(*args):
            r = f(*args)
            self.calls.append([name, list(args), r])
            return r
        return wrapped


def load_reference(checkout: str):
    path = os.path.join(checkout, "omnidata_tools", "torch", "data", "augmentation.py")
    sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
    spec = importlib.util.spec_from_file_location("reference_augmentation", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_recorded(mod, method_name, call):
    """call() under a recorder: (recorded random calls, locals of the reference's frame of `method_name` when it ended, result or
    None, the exception's text or None)"""
    rec = RecordingRandom()
    mod.random = rec
    seen = {}

    def profile(frame, event, arg):
        if event == "return" and frame.f_code.co_name == method_name:
            seen.update({k: v for k, v in frame.f_locals.items() if isinstance(v, (int, float, str))})

    result = error = None
    sys.setprofile(profile)
    try:
        result = call()
    except Exception as e:   # the reference's own failure (NameError without kornia, ValueError of an empty randrange)
        error = f"{type(e).__name__}: {e}"
    finally:
        sys.setprofile(None)
        mod.random = random
    return rec.calls, seen, result, error


def resize_record(seed, calls, seen, error):
    off = [seen["min_x"], seen["min_y"]] if "min_x" in seen else None
    return {"seed": seed, "calls": calls, "method": seen.get("resize_method"), "size": [seen.get("h"), seen.get("w")],
            "offset": off, "completed": error is None, "error": error}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--omnidata", required=True, help="checkout of the reference repository")
    args = ap.parse_args()
    mod = load_reference(args.omnidata)
    aug = mod.Augmentation()
    rng = np.random.default_rng(20261020)
    q = lambda *shape: torch.from_numpy((rng.integers(0, 257, shape) / 256.0).astype(np.float32))
    inputs = {"rgb": q(2, 3, 72, 80), "depth_zbuffer": q(2, 1, 72, 80),
              "mask_valid": torch.from_numpy((rng.random((2, 1, 72, 80)) < 0.7).astype(np.float32))}
    np.savez_compressed(os.path.join(OUT, "augment_resize_small_inputs.npz"), **{k: v.numpy() for k, v in inputs.items()})

    small, outputs = [], {}
    for seed in SEEDS:
        random.seed(seed)
        batch = {k: v.clone() for k, v in inputs.items()}
        calls, seen, result, error = run_recorded(mod, "resize_augmentation", lambda: aug.resize_augmentation(batch, TASKS, fixed_size=48))
        rec = resize_record(seed, calls, seen, error)
        if error is None:   # seeds with the same decisions have the same output: it is stored once, 'output_seed' says where
            twin = next((r for r in small if r["completed"] and (r["method"], r["size"], r["offset"]) ==
                         (rec["method"], rec["size"], rec["offset"])), None)
            rec["output_seed"] = seed if twin is None else twin["output_seed"]
            if twin is None:
                for t in TASKS:
                    outputs[f"s{seed}_{t}"] = result[t].numpy()
            else:
                assert all(np.array_equal(outputs[f"s{twin['output_seed']}_{t}"], result[t].numpy()) for t in TASKS)
        small.append(rec)
    for k in range(0, len(SEEDS), 8):
        part = {n: a for n, a in outputs.items() if k <= int(n[1:].split("_")[0]) < k + 8}
        path = os.path.join(OUT, f"augment_resize_small_outputs_{k // 8}.npz")
        np.savez_compressed(path, **part)
        print(f"{path}: {os.path.getsize(path)} B, {len(part) // len(TASKS)} outputs")
        assert os.path.getsize(path) < LIMIT, path

    free = []
    for seed in SEEDS:
        random.seed(seed)
        batch = {"depth_zbuffer": torch.zeros(1, 1, 512, 512)}
        calls, seen, _, error = run_recorded(mod, "resize_augmentation", lambda: aug.resize_augmentation(batch, ["depth_zbuffer"]))
        free.append(resize_record(seed, calls, seen, error))

    made = []

    def stand_in(name):
        def make(*a, **kw):
            made.append([name, [list(v) if isinstance(v, tuple) else v for v in a], kw])
            return lambda x: x
        return make

    for name in ("ColorJitter", "RandomSharpness", "RandomMotionBlur", "RandomGaussianBlur"):
        setattr(mod, name, stand_in(name))
    rgb = []
    for seed in SEEDS:
        random.seed(seed)
        made.clear()
        batch = {"positive": {"rgb": inputs["rgb"]}}
        calls, _, _, error = run_recorded(mod, "augment_rgb", lambda: aug.augment_rgb(batch))
        rgb.append({"seed": seed, "calls": calls, "made": [m for m in made if m[0] != "ColorJitter"], "error": error})

    path = os.path.join(OUT, "augment_resize_decisions.npz")
    np.savez_compressed(path, small=np.array(json.dumps(small)), free512=np.array(json.dumps(free)), rgb=np.array(json.dumps(rgb)))
    print(f"{path}: {os.path.getsize(path)} B")
    assert os.path.getsize(path) < LIMIT
    for name, recs in (("small", small), ("free512", free)):
        print(name, "complete:", [r["seed"] for r in recs if r["completed"]], "raise:", [r["seed"] for r in recs if not r["completed"]])


if __name__ == "__main__":
    main()
