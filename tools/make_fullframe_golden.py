"""Writes tests/golden/fullframe_sizes.json: the network size the reference picks for an image of a given size.

    python tools/make_fullframe_golden.py --omnidata <checkout of EPFL-VILAB/omnidata>

Imports omnidata_tools/torch/modules/midas/transforms.py from that checkout at run time and calls
Resize(size, size, keep_aspect_ratio=True, ensure_multiple_of=multiple, resize_method='lower_bound').get_size(w, h)
(transforms.py:94-160).  The module needs cv2 only for the INTER_* constants of its defaults, so a stub module with those four
names stands in for it; nothing of the checkout is copied here.  The table holds rows [w, h, size, multiple, net_w, net_h]:
ten fixed image sizes at (384, 32), a few hundred random ones, and rows for size 64 and for multiple 64.
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import random
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "fullframe_sizes.json")
FIXED = [(640, 512), (1920, 1080), (4000, 3000), (3000, 4000), (400, 400), (777, 385), (50, 33), (2048, 640), (1000, 999),
         (1039, 640)]


def load_reference(checkout: str):
    if "cv2" not in sys.modules:
        stub = types.ModuleType("cv2")
        stub.INTER_NEAREST, stub.INTER_LINEAR, stub.INTER_CUBIC, stub.INTER_AREA = 0, 1, 2, 3
        sys.modules["cv2"] = stub
    path = os.path.join(checkout, "omnidata_tools", "torch", "modules", "midas", "transforms.py")
    spec = importlib.util.spec_from_file_location("reference_midas_transforms", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--omnidata", required=True)
    args = ap.parse_args()
    ref = load_reference(args.omnidata)

    def row(w, h, size, multiple):
        nw, nh = ref.Resize(size, size, keep_aspect_ratio=True, ensure_multiple_of=multiple,
                            resize_method="lower_bound").get_size(w, h)
        return [w, h, size, multiple, int(nw), int(nh)]

    rng = random.Random(0)
    rows = [row(w, h, 384, 32) for w, h in FIXED]
    for _ in range(300):
        rows.append(row(rng.randint(1, 6000), rng.randint(1, 6000), 384, 32))
    for _ in range(60):   # sides near the size, where rounding and the lower bound meet
        rows.append(row(rng.randint(350, 450), rng.randint(350, 450), 384, 32))
    for _ in range(80):
        rows.append(row(rng.randint(1, 3000), rng.randint(1, 3000), 64, 32))
    for _ in range(80):
        rows.append(row(rng.randint(1, 6000), rng.randint(1, 6000), 384, 64))
    for _ in range(40):
        rows.append(row(rng.randint(1, 3000), rng.randint(1, 3000), 512, 64))
    with open(OUT, "w") as f:
        json.dump({"columns": ["w", "h", "size", "multiple", "net_w", "net_h"], "rows": rows}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {len(rows)} rows")


if __name__ == "__main__":
    main()
