"""Writes tests/golden/vnl_*.npz: inputs, triples, loss and fp32 autograd gradients of the reference's virtual normal loss on
the CPU.

    python tools/make_vnl_golden.py --omnidata <checkout of EPFL-VILAB/omnidata>

Loads omnidata_tools/torch/losses/virtual_normal_loss.py from that checkout at run time (with numpy.int = int, which the
module needs on numpy >= 1.24); nothing of it is copied here.  Each case stores first, second [B,1,H,W] fp32 (the two
arguments of VNL_Loss.forward in its order), fx, fy, delta_z, select, the seed given to np.random.seed before the call, the
six index arrays of select_index() under that seed and the next np.random.random() after it, the loss, K, the fp32
autograd gradients with respect to BOTH arguments, the mask of filter_mask and the compacted point groups of
select_points_groups.  Also, for the GPU tests' bounds: e_ref_first / e_ref_second = max |g_reference - g_fp64| / max |g_fp64|
against fp64 autograd of tests/vnl_restatement.py outside the kink pixels.

Every case must keep its borderline triples (tests/vnl_restatement.py: a mask comparison decided by less than rounding)
under 0.1 % of the triples, with the reference's mask equal to the restatement's on all others, and its kink pixels under
1 % of the pixels with a gradient: asserted here; a seed that does not is skipped for the next one.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vnl_restatement as rs  # noqa: E402


def load_reference(checkout: str):
    np.int = int  # the reference's select_index uses the alias numpy removed in 1.24
    path = os.path.join(checkout, "omnidata_tools", "torch", "losses", "virtual_normal_loss.py")
    spec = importlib.util.spec_from_file_location("reference_virtual_normal_loss", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def smooth(rng, B, H, W, lo, hi, k=6):
    """[B,1,H,W] fp32 smooth random field in [lo, hi] (bilinear upsampling of a coarse grid)."""
    g = torch.from_numpy(rng.random((B, 1, k, k)).astype(np.float32))
    f = torch.nn.functional.interpolate(g, size=(H, W), mode="bilinear", align_corners=True)
    f = (f - f.amin((2, 3), keepdim=True)) / (f.amax((2, 3), keepdim=True) - f.amin((2, 3), keepdim=True))
    return (lo + (hi - lo) * f).float().contiguous()


def pair(rng, B, H, W, lo, hi):
    """a depth and a second one that differs from it by a smooth field and noise, both in about [lo, hi]"""
    t = smooth(rng, B, H, W, lo, hi)
    p = 0.8 * t + 0.2 * smooth(rng, B, H, W, lo, hi) + torch.from_numpy(rng.normal(0, 0.01 * (hi - lo), t.shape).astype(np.float32))
    return t, p.clamp(lo * 0.5, hi * 1.5).float().contiguous()


def run(ref, first, second, fx, fy, seed, select=True, delta_z=0.0001):
    H, W = first.shape[-2:]
    mod = ref.VNL_Loss(fx, fy, (H, W), delta_z=delta_z)
    np.random.seed(seed)
    p123 = mod.select_index()
    after = np.random.random()
    # the reference's own mask and groups under the same draw
    mask, _ = mod.filter_mask(p123, mod.transfer_xyz(first))
    np.random.seed(seed)
    groups_first, groups_second = mod.select_points_groups(first, second)
    a, b = first.clone().requires_grad_(True), second.clone().requires_grad_(True)
    np.random.seed(seed)
    loss = mod(a, b, select=select)
    K = int(mask.sum())
    if K > 0:
        loss.backward()
    ga = a.grad if a.grad is not None else torch.zeros_like(a)
    gb = b.grad if b.grad is not None else torch.zeros_like(b)
    # the conditions on the inputs (module docstring)
    p = rs.linear_indices(p123, W)
    out = rs.forward(first[:, 0], second[:, 0], p, fx, fy, delta_z, select)
    nb = int(out["borderline"].sum())
    if nb > 0.001 * mask.numel() or not torch.equal(mask[~out["borderline"]], out["keep"][~out["borderline"]]):
        print(f"  seed {seed}: {nb} borderline triples of {mask.numel()}, or a mask that differs outside them; next seed")
        return None
    g64 = rs.fp64_gradients(first[:, 0], second[:, 0], p, fx, fy, out)
    kink = rs.kink_pixels(p, out, first[:, 0].shape)
    e_ref = []
    for g32, g in ((ga[:, 0], g64[0]), (gb[:, 0], g64[1])):
        if int((kink & (g != 0)).sum()) > 0.01 * int((g != 0).sum()):
            print(f"  seed {seed}: {int((kink & (g != 0)).sum())} kink pixels of {int((g != 0).sum())}; next seed")
            return None
        gmax = g.abs().max().item()
        e_ref.append((g32.double() - g)[~kink].abs().max().item() / gmax if gmax > 0 else 0.0)
    print(f"  seed {seed}: K {K} of {mask.numel()}, loss {loss.item():.7g}, borderline {nb}, kink pixels {int(kink.sum())}, "
          f"e_ref {e_ref[0]:.3e} {e_ref[1]:.3e}")
    d = dict(first=first, second=second, fx=np.float64(fx), fy=np.float64(fy), delta_z=np.float64(delta_z),
             select=np.int64(bool(select)), seed=np.int64(seed), after=np.float64(after), loss=loss.detach(), K=np.int64(K),
             grad_first=ga, grad_second=gb, mask=mask, groups_first=groups_first.detach()[0], groups_second=groups_second.detach()[0],
             e_ref_first=np.float64(e_ref[0]), e_ref_second=np.float64(e_ref[1]))
    d.update({k: np.asarray(v).astype(np.int32) for k, v in p123.items()})
    return d


def save(name, ref, first, second, fx, fy, seed, **kw):
    print(name)
    for s in range(seed, seed + 20):
        d = run(ref, first, second, fx, fy, s, **kw)
        if d is not None:
            break
    else:
        raise SystemExit(f"{name}: no seed keeps the borderline triples and kink pixels under their caps")
    arrs = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    path = os.path.join(OUT, f"vnl_{name}.npz")
    np.savez_compressed(path, **arrs)
    print(f"  {path}: {os.path.getsize(path)} B")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--omnidata", required=True, help="checkout of the reference repository")
    args = ap.parse_args()
    ref = load_reference(args.omnidata)
    rng = np.random.default_rng(20261016)
    torch.set_num_threads(4)

    # 1. the regime of train_depth.py: depths in [0, 1], fx = fy = 1, VNL_Loss(gt, pred)
    t, p = pair(rng, 3, 48, 64, 0.05, 1.0)
    save("unit", ref, t, p, 1.0, 1.0, 100)
    # 2. metric depths with a realistic focal length, odd size
    t, p = pair(rng, 3, 37, 53, 0.5, 8.0)
    save("metric_odd", ref, t, p, 50.0, 48.0, 200)
    # 3. the slot order of train_depth.py:272: the prediction first (the masks come from it)
    t, p = pair(rng, 2, 32, 40, 0.05, 1.0)
    save("pred_first", ref, p, t, 1.0, 1.0, 300)
    # 4. exact zeros in the second argument (:144), values <= delta_z in the first (mask_pad)
    t, p = pair(rng, 2, 32, 40, 0.05, 1.0)
    hole = torch.from_numpy(rng.random(t.shape))
    t = torch.where(hole < 0.04, torch.zeros_like(t), torch.where(hole < 0.08, torch.full_like(t, 0.00005), t))
    p = torch.where(torch.from_numpy(rng.random(p.shape)) < 0.08, torch.zeros_like(p), p)
    save("zeros", ref, t, p, 1.0, 1.0, 400)
    # 5. select = False
    t, p = pair(rng, 2, 32, 40, 0.05, 1.0)
    save("noselect", ref, t, p, 1.0, 1.0, 500, select=False)
    # 6. first == second: every loss 0, all ties
    t, _ = pair(rng, 2, 32, 40, 0.05, 1.0)
    save("same", ref, t, t.clone(), 1.0, 1.0, 600)
    # 7. no triple survives: the first argument is 0 everywhere
    t, p = pair(rng, 2, 24, 32, 0.05, 1.0)
    save("none", ref, torch.zeros_like(t), p, 1.0, 1.0, 700)


if __name__ == "__main__":
    main()
