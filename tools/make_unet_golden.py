"""Writes tests/golden/unet_*.npz: the reference's version-1 UNet run on the CPU in fp32 with seeded weights and inputs.

    python tools/make_unet_golden.py --omnidata <checkout of EPFL-VILAB/omnidata>

Imports omnidata_tools/torch/modules/unet.py from that checkout at run time (plain torch); nothing of it is copied here.
The weights (75.5 M values) and inputs are regenerated from the seed by tests/unet_restatement.py and never stored.

Every file holds seed, out_channels, shape [B, out, H, W], y (the reference's fp32 output), parts, and e_model_fp16 /
e_model_bf16 = max |rounding model - reference output| of that case, computed here on the CPU with
tests/unet_restatement.py unet_forward_rounded: the distance the engine's storage roundings alone put between it and the
reference.  It also prints max |unet_forward_fp32 - reference| (the restatement against the reference's own code).
A case whose y would exceed 1 MiB is written as two files split by rows (unet_restatement.load_golden joins them).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")
LIMIT = 1000 * 1024   # bytes of y per file (a committed file stays below 1 MiB)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--omnidata", required=True, help="checkout of the reference repository")
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.omnidata, "omnidata_tools", "torch"))
    from modules.unet import UNet   # the reference's module, imported, not copied
    from tests.unet_restatement import GOLDEN_CASES, unet_forward_fp32, unet_forward_rounded, unet_input, unet_random_state_dict

    torch.manual_seed(0)
    for name, (seed, oc, B, H, W) in GOLDEN_CASES.items():
        if args.only and args.only != name:
            continue
        sd = unet_random_state_dict(seed, oc)
        x = unet_input(seed, B, H, W)
        ref = UNet(downsample=6, in_channels=3, out_channels=oc).eval()
        ref.load_state_dict(sd, strict=True)
        with torch.no_grad():
            y = ref(x).float()
        e32 = float((unet_forward_fp32(sd, x) - y).abs().max())
        e = {d: float((unet_forward_rounded(sd, x, d) - y).abs().max()) for d in ("fp16", "bf16")}
        ya = y.numpy()
        fields = dict(seed=np.int64(seed), out_channels=np.int64(oc), shape=np.array(ya.shape, dtype=np.int64),
                      e_model_fp16=np.float64(e["fp16"]), e_model_bf16=np.float64(e["bf16"]))
        if ya.nbytes > LIMIT:
            split = H // 2
            np.savez(os.path.join(OUT, name + ".npz"), y=ya[:, :, :split], parts=np.int64(2), **fields)
            np.savez(os.path.join(OUT, name + "_part2.npz"), y=ya[:, :, split:])
        else:
            np.savez(os.path.join(OUT, name + ".npz"), y=ya, parts=np.int64(1), **fields)
        print(f"{name}: range [{ya.min():.3f}, {ya.max():.3f}]  restatement fp32 {e32:.3e}  e_model fp16 {e['fp16']:.3e}  bf16 {e['bf16']:.3e}")


if __name__ == "__main__":
    main()
