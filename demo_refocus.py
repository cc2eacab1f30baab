"""3D refocus augmentation of a folder of images (the reference's omnidata_tools/torch/demo_refocus.py), on the GPU.

    python demo_refocus.py --input_path <dir> --output_path <dir> [--num_quantiles 10] [--min_aperture 0.001]
                           [--max_aperture 6] [--seed S]

Every file of --input_path whose name contains 'rgb' is refocused with its depth file, path.replace('rgb',
'depth_euclidean') (over the whole path, as the reference does), and written as <name>_refocused.png.
  rgb  : Resize(512, BILINEAR) on the shorter side, ToTensor, [:3], grey repeated to 3 channels
  depth: Resize(512, NEAREST), fp32(v) / 65535, / fp32(8000 / 65535)   (data/transforms.py, task_configs.py)
Two deliberate differences: --num_quantiles is parsed as an int (the reference passes the string on and fails whenever
the flag is given), and 16-bit PNGs are read as unsigned values (no int16 wrap-around).  --seed makes a run reproducible.
"""
from __future__ import annotations

import argparse
import glob
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from omnidata_amd.preprocess import resize_shorter, to_tensor  # noqa: E402
from omnidata_amd.refocus import RefocusImageAugmentation  # noqa: E402

DEPTH_MAX = 8000.0 / (2 ** 16 - 1)  # task_configs.py: depth_euclidean clamp_to


def load_rgb(path: str, size: int = 512) -> torch.Tensor:
    """[1, 3, h, w] fp32 in [0, 1]."""
    t = to_tensor(resize_shorter(Image.open(path), size, Image.BILINEAR))[:3].unsqueeze(0)
    if t.shape[1] == 1:
        t = t.repeat_interleave(3, 1)
    return t


def load_depth(path: str, size: int = 512) -> torch.Tensor:
    """[1, 1, h, w] fp32: 16-bit depth (units of 1/65535 of the sensor range) rescaled so that 8000 / 65535 -> 1."""
    img = resize_shorter(Image.open(path), size, Image.NEAREST)
    a = np.array(img)
    if a.ndim == 2:
        a = a[:, :, None]
    t = torch.from_numpy(a.astype(np.int64) if a.dtype != np.uint8 else a).permute(2, 0, 1)
    t = t.float().div(255.0) if a.dtype == np.uint8 else t.float()  # ToTensor
    t = t.float() / (2 ** 16 - 1.0)
    t = t / torch.tensor(DEPTH_MAX, dtype=torch.float32)             # Normalize([0], [8000 / 65535])
    return t[:1].unsqueeze(0).contiguous()


def to_u8(x: torch.Tensor) -> Image.Image:
    """ToPILImage of a [3, H, W] float tensor: mul(255).byte() (truncation)."""
    return Image.fromarray(x.detach().mul(255).byte().permute(1, 2, 0).cpu().numpy())


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="Visualize 3D refocus augmentation")
    p.add_argument("--num_quantiles", type=int, default=10, help="number of quantiles in the blur stack: more is better, but slower")
    p.add_argument("--min_aperture", type=float, default=0.001, help="smallest aperture to use")
    p.add_argument("--max_aperture", type=float, default=6, help="largest aperture to use")
    p.add_argument("--input_path", required=True, help="folder with *rgb* images and their depth_euclidean images")
    p.add_argument("--output_path", required=True, help="where the refocused images are written")
    p.add_argument("--seed", type=int, default=None, help="torch seed of the focus / aperture draws")
    args = p.parse_args(argv)
    if not os.path.isdir(args.input_path):
        print("invalid file path!")
        return 1
    if not torch.cuda.is_available():
        print("demo_refocus.py needs an MI355X (omnidata_amd has no CPU path)")
        return 1
    os.makedirs(args.output_path, exist_ok=True)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    device = torch.device("cuda")
    aug = RefocusImageAugmentation(args.num_quantiles, float(args.min_aperture), float(args.max_aperture))
    for f in sorted(glob.glob(args.input_path + "/*")):
        name = os.path.splitext(os.path.basename(f))[0]
        if "rgb" not in name:
            continue
        save_path = os.path.join(args.output_path, name + "_refocused.png")
        print(f"Reading input {f} ...")
        rgb = load_rgb(f).to(device)
        depth = load_depth(f.replace("rgb", "depth_euclidean")).to(device)
        out = aug(rgb, depth)
        print(f"Writing output {save_path} ...")
        to_u8(out[0]).save(save_path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
