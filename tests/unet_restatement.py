"""The reference's version-1 UNet (omnidata_tools/torch/modules/unet.py:8-105) restated in torch ops, seeded weights and
inputs for it, and the ROUNDING MODEL of the engine's forward (omnidata_amd/csrc/unet_engine.hip).  No reference code is
imported; tools/make_unet_golden.py pins `unet_forward_fp32` to the reference's own module.

Where the engine rounds to its 16-bit storage type (`unet_forward_rounded` rounds at exactly these points, arithmetic fp32):
  * the input image, when the first layer's im2col stores it;
  * the weights of every 3x3 convolution (biases, norm vectors and last_conv2 stay fp32);
  * the raw output of every 3x3 convolution (fp32 accumulator + bias), stored before normalisation;
  * GroupNorm statistics are taken AFTER that store's rounding (over the stored values), combined in double; mean and
    rstd are fp32;
  * relu(gn(x)) = max(x * a + c, 0) with a = rstd * gamma, c = beta - mean * a, stored rounded -- except behind last_conv1,
    where the normalised values stay fp32 and feed last_conv2 (fp32 weights) directly;
  * the 2x2 max-pool picks among stored values (no rounding of its own);
  * the bilinear x2 up-sample (fp32 blend of stored values) is stored rounded.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

DOWNSAMPLE = 6
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def unet_state_dict_spec(out_channels: int = 3):
    """[(key, shape)] in the reference's state-dict order (174 entries)."""
    spec = []

    def conv(name, cin, cout, k=3):
        spec.append((name + ".weight", (cout, cin, k, k)))
        spec.append((name + ".bias", (cout,)))

    def norm(name, c):
        spec.append((name + ".weight", (c,)))
        spec.append((name + ".bias", (c,)))

    def block(pre, cin, cout):
        for j in (1, 2, 3):
            conv(f"{pre}.conv{j}", cin if j == 1 else cout, cout)
            norm(f"{pre}.bn{j}", cout)

    block("down1", 3, 16)
    for i in range(DOWNSAMPLE):
        block(f"down_blocks.{i}", 2 ** (4 + i), 2 ** (5 + i))
    for j in (1, 2, 3):
        conv(f"mid_conv{j}", 1024, 1024)
        norm(f"bn{j}", 1024)
    for i in range(DOWNSAMPLE):
        block(f"up_blocks.{i}", 2 ** (4 + i) + 2 ** (5 + i), 2 ** (4 + i))
    conv("last_conv1", 16, 16)
    norm("last_bn", 16)
    conv("last_conv2", 16, out_channels, 1)
    return spec


def unet_random_state_dict(seed: int, out_channels: int = 3):
    """Seeded weights from numpy's RandomState (stable across torch versions): He-scaled convolutions (std sqrt(2 / fan_in);
    last_conv2, which has no ReLU behind it, std 2 / sqrt(fan_in) so that the output spans a few units), biases in
    [-0.1, 0.1], norm weights in [0.5, 1.5], norm biases in [-0.3, 0.3]."""
    rs = np.random.RandomState(1000 + seed)
    sd = {}
    for key, shape in unet_state_dict_spec(out_channels):
        if len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            std = 2.0 / np.sqrt(fan_in) if key.startswith("last_conv2") else np.sqrt(2.0 / fan_in)
            a = rs.standard_normal(shape) * std
        elif ".bn" in key or key.startswith(("bn", "last_bn")):
            a = rs.uniform(0.5, 1.5, shape) if key.endswith(".weight") else rs.uniform(-0.3, 0.3, shape)
        else:
            a = rs.uniform(-0.1, 0.1, shape)
        sd[key] = torch.from_numpy(a.astype(np.float32))
    return sd


def unet_input(seed: int, B: int, H: int, W: int) -> torch.Tensor:
    """[B,3,H,W] fp32 in [0, 1]: 8x8 blocks of colour plus pixel noise (what get_transform('rgb') hands the model)."""
    rs = np.random.RandomState(2000 + seed)
    coarse = np.kron(rs.rand(B, 3, H // 8, W // 8), np.ones((1, 1, 8, 8)))
    x = 0.7 * coarse + 0.3 * rs.rand(B, 3, H, W)
    return torch.from_numpy(x.astype(np.float32)).clamp_(0.0, 1.0)


def _forward(sd, x, rnd):
    """The forward with `rnd` applied wherever the engine stores a 16-bit value (identity: the fp32 forward)."""
    exact = rnd is None
    r = (lambda t: t) if exact else rnd

    def conv(name, t):
        return r(F.conv2d(t, r(sd[name + ".weight"].float()), sd[name + ".bias"].float(), padding=1))

    def gn(name, t, store=True):
        g, b = sd[name + ".weight"].float(), sd[name + ".bias"].float()
        if exact:
            return F.relu(F.group_norm(t, 8, g, b, 1e-5))
        B, C = t.shape[:2]
        t64 = t.double().reshape(B, 8, -1)
        mean = t64.mean(-1)
        var = ((t64 * t64).mean(-1) - mean * mean).clamp_min(0.0)
        rstd = (1.0 / torch.sqrt(var + 1e-5)).float().repeat_interleave(C // 8, 1)    # [B, C]
        mean = mean.float().repeat_interleave(C // 8, 1)
        a = rstd * g[None]
        c = b[None] - mean * a
        y = F.relu(t * a[:, :, None, None] + c[:, :, None, None])
        return r(y) if store else y

    def block(pre, t):
        for j in (1, 2, 3):
            t = gn(f"{pre}.bn{j}", conv(f"{pre}.conv{j}", t))
        return t

    t = block("down1", r(x.float()))
    skips = [t]
    for i in range(DOWNSAMPLE):
        t = F.max_pool2d(block(f"down_blocks.{i}", t), 2, 2)
        skips.append(t)
    for j in (1, 2, 3):
        t = gn(f"bn{j}", conv(f"mid_conv{j}", t))
    for i in reversed(range(DOWNSAMPLE)):
        up = r(F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False))
        t = block(f"up_blocks.{i}", torch.cat((up, skips[i]), 1))
    t = gn("last_bn", conv("last_conv1", t), store=False)
    return F.conv2d(t, sd["last_conv2.weight"].float(), sd["last_conv2.bias"].float())


@torch.no_grad()
def unet_forward_fp32(sd, x):
    """The reference's arithmetic in torch ops: [B,3,H,W] fp32 -> [B,out,H,W] fp32."""
    return _forward(sd, x, None)


@torch.no_grad()
def unet_forward_rounded(sd, x, dtype: str):
    """The rounding model: the same forward with the weights and every activation the engine stores rounded to `dtype`
    ('fp16' / 'bf16') at the points listed in the module docstring."""
    tdt = TDT[dtype]
    return _forward(sd, x, lambda t: t.to(tdt).float())


class TorchUNet(torch.nn.Module):
    """`unet_forward_fp32` as a module (parameters under the reference's names): `.half().cuda()` of it is the torch 16-bit
    yardstick of tools/unet_bench.py."""

    def __init__(self, sd):
        super().__init__()
        self.params = torch.nn.ParameterDict({k.replace(".", "__"): torch.nn.Parameter(v.clone(), requires_grad=False) for k, v in sd.items()})

    def forward(self, x):
        p = {k.replace("__", "."): v for k, v in self.params.items()}

        def block(pre, t):
            for j in (1, 2, 3):
                t = F.conv2d(t, p[f"{pre}.conv{j}.weight"], p[f"{pre}.conv{j}.bias"], padding=1)
                t = F.relu(F.group_norm(t, 8, p[f"{pre}.bn{j}.weight"], p[f"{pre}.bn{j}.bias"], 1e-5))
            return t

        t = block("down1", x)
        skips = [t]
        for i in range(DOWNSAMPLE):
            t = F.max_pool2d(block(f"down_blocks.{i}", t), 2, 2)
            skips.append(t)
        for j in (1, 2, 3):
            t = F.conv2d(t, p[f"mid_conv{j}.weight"], p[f"mid_conv{j}.bias"], padding=1)
            t = F.relu(F.group_norm(t, 8, p[f"bn{j}.weight"], p[f"bn{j}.bias"], 1e-5))
        for i in reversed(range(DOWNSAMPLE)):
            t = F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)
            t = block(f"up_blocks.{i}", torch.cat((t, skips[i]), 1))
        t = F.conv2d(t, p["last_conv1.weight"], p["last_conv1.bias"], padding=1)
        t = F.relu(F.group_norm(t, 8, p["last_bn.weight"], p["last_bn.bias"], 1e-5))
        return F.conv2d(t, p["last_conv2.weight"], p["last_conv2.bias"])


# ---- goldens of tools/make_unet_golden.py
GOLDEN_CASES = {   # name: (seed, out_channels, B, H, W)
    "unet_normal_seed0_64x64": (0, 3, 2, 64, 64),
    "unet_normal_seed1_128x192": (1, 3, 1, 128, 192),
    "unet_depth_seed2_64x128": (2, 1, 3, 64, 128),
    "unet_normal_seed3_384x384": (3, 3, 1, 384, 384),
}


def load_golden(golden_dir, name):
    """{'seed', 'out_channels', 'shape', 'y', 'e_model_fp16', 'e_model_bf16'}.  A case whose fp32 output exceeds the size a
    committed file may have is stored as <name>.npz (rows [0, split) of y and every other field) and <name>_part2.npz (the
    remaining rows)."""
    import os
    z = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    y = z["y"]
    if int(z["parts"]) == 2:
        y = np.concatenate([y, np.load(os.path.join(golden_dir, name + "_part2.npz"))["y"]], axis=2)
    z["y"] = y
    assert tuple(y.shape) == tuple(int(v) for v in z["shape"])
    return z
