"""Writes tests/golden/normal_*.npz: inputs, losses and fp32 autograd gradients of the reference's surface-normal objective on
the CPU.

    python tools/make_normal_golden.py --omnidata <checkout of EPFL-VILAB/omnidata>

Loads omnidata_tools/torch/losses/masked_losses.py from that checkout at run time, and takes make_valid_mask out of
omnidata_tools/torch/train_normal.py without importing it (the module needs pytorch_lightning): the file is parsed with ast,
that one FunctionDef is compiled and called with self=None.  Nothing of the checkout is copied here.

Loss cases store pred, target [B,3,H,W] fp32, mask [B,1,H,W] bool, flags and l1_weight (include/dptx.h DPTX_NORMAL_*), and
from the reference (train_normal.py:251-258: clamp where the flags say so, masked_l1_loss and masked_cosine_angular_loss on
the mask repeated over the channels, cos + l1_weight * l1): losses = (total, l1, cos) in fp32, losses64 = the same functions
on .double() inputs, grad_total and grad_cos = fp32 autograd of the total and of the cosine loss alone, and e_ref / e_ref_cos =
the scaled error (tests/normal_restatement.py scaled_error) of those two gradients against the restatement's fp64 autograd:
the reference's own fp32 error, which the GPU tests' bound is made of.
"""
from __future__ import annotations

import argparse
import ast
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import normal_restatement as rs  # noqa: E402


def load_reference(checkout: str):
    base = os.path.join(checkout, "omnidata_tools", "torch")
    spec = importlib.util.spec_from_file_location("reference_masked_losses", os.path.join(base, "losses", "masked_losses.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    path = os.path.join(base, "train_normal.py")
    tree = ast.parse(open(path).read(), filename=path)
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "make_valid_mask")
    ns = {"F": torch.nn.functional, "torch": torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return mod, ns["make_valid_mask"]


def reference(ref, pred, target, mask, flags, l1_weight, dtype, grads):
    """train_normal.py:251-258 in `dtype` -> losses (total, l1, cos) and, with grads, the gradients of total and of cos"""
    m3 = mask.repeat_interleave(3, 1)
    t = target.to(dtype)
    out = []
    for which in ("total", "cos"):
        a = pred.to(dtype).clone().requires_grad_(grads)
        p = torch.clamp(a, 0, 1) if flags & rs.CLAMP_PRED else a
        l1 = ref.masked_l1_loss(p, t, m3)
        cos = ref.masked_cosine_angular_loss(p, t, m3)
        total = cos + l1_weight * l1
        g = None
        if grads:
            (total if which == "total" else cos).backward()
            g = a.grad if a.grad is not None else torch.zeros_like(a)
        out.append((torch.stack([total, l1, cos]).detach(), g))
    return out[0][0], out[0][1], out[1][1]


def save_loss(name, ref, pred, target, mask, flags, l1_weight=10.0):
    pred, target = pred.float().contiguous(), target.float().contiguous()
    losses, g_total, g_cos = reference(ref, pred, target, mask, flags, l1_weight, torch.float32, True)
    losses64, _, _ = reference(ref, pred, target, mask, flags, l1_weight, torch.float64, False)
    e = {}
    for key, g, fl, gl in (("e_ref", g_total, flags | rs.L1 | rs.COS, (1.0, 0.0, 0.0)), ("e_ref_cos", g_cos, (flags & rs.CLAMP_PRED) | rs.COS, (0.0, 0.0, 1.0))):
        out = rs.evaluate(pred, target, mask[:, 0], fl, l1_weight, gl)
        e[key] = rs.scaled_error(g, out["grad"], rs.gradient_scale(out, fl, l1_weight, gl)) if out["N"] else 0.0
    path = os.path.join(OUT, f"normal_{name}.npz")
    np.savez_compressed(path, pred=pred.numpy(), target=target.numpy(), mask=mask.numpy(), flags=np.int64(flags),
                        l1_weight=np.float64(l1_weight), losses=losses.numpy(), losses64=losses64.numpy(), grad_total=g_total.numpy(),
                        grad_cos=g_cos.numpy(), e_ref=np.float64(e["e_ref"]), e_ref_cos=np.float64(e["e_ref_cos"]))
    print(f"{name}: N {int(mask.sum())}, losses {losses.tolist()}, e_ref {e['e_ref']:.3e} (cos alone {e['e_ref_cos']:.3e}), "
          f"{os.path.getsize(path)} B")


def normals(rng, B, H, W):
    """targets 0.5 n + 0.5 for random unit n"""
    n = rng.normal(size=(B, 3, H, W))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return torch.from_numpy((0.5 * n + 0.5).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--omnidata", required=True, help="checkout of the reference repository")
    args = ap.parse_args()
    ref, make_valid_mask = load_reference(args.omnidata)
    rng = np.random.default_rng(20261018)
    torch.set_num_threads(4)
    both = rs.L1 | rs.COS

    def noise(shape, s):
        return torch.from_numpy(rng.normal(0, s, shape).astype(np.float32))

    def mask_of(B, H, W, keep=0.75):
        return torch.from_numpy(rng.random((B, 1, H, W)) < keep)

    # 1. the regime of train_normal.py: predictions already inside [0, 1]
    t = normals(rng, 2, 32, 48)
    save_loss("unit", ref, (t + noise(t.shape, 0.15)).clamp(0, 1), t, mask_of(2, 32, 48), both)
    # 2. odd H*W, an unclamped prediction with values outside [0, 1] (the inner clamp of 2 p - 1 works)
    t = normals(rng, 2, 37, 53)
    save_loss("odd", ref, t + noise(t.shape, 0.3), t, mask_of(2, 37, 53), both)
    # 3. raw predictions outside [0, 1], clamped before the reference call: the gradient goes through the clamp
    t = normals(rng, 2, 24, 32)
    p = t + noise(t.shape, 0.4)
    p[0, :, 0, :8] = torch.tensor([0.0, 1.0, -0.0, 1.0, 0.0, 1.0, 0.0, 1.0])      # exactly on the ends: the gradient passes
    save_loss("clamp", ref, p, t, mask_of(2, 24, 32), both | rs.CLAMP_PRED)
    # 4. degenerate pixels, all inside the mask
    t = normals(rng, 2, 24, 32)
    p = (t + noise(t.shape, 0.15)).clamp(0, 1)
    m = mask_of(2, 24, 32)
    p[:, :, 0, :] = 0.5                                                           # the zero vector: gradient -2 yh / (eps N)
    sign = torch.from_numpy(rng.choice([-1.0, 1.0], size=(2, 3, 32)).astype(np.float32))
    p[:, :, 1, :] = 0.5 + 1e-6 * sign                                             # next to it: a tiny norm
    p[:, :, 2, :] = t[:, :, 2, :]                                                 # pred == target
    t[:, :, 3, :] = 0.5                                                           # a zero target vector
    p[:, :, 4, :16] = 0.5                                                         # both zero
    t[:, :, 4, :16] = 0.5
    m[:, :, :5, :] = True
    save_loss("degenerate", ref, p, t, m, both)
    # 5. an empty mask
    t = normals(rng, 1, 8, 12)
    save_loss("empty", ref, (t + noise(t.shape, 0.15)).clamp(0, 1), t, torch.zeros(1, 1, 8, 12, dtype=torch.bool), both)

    # 6. the flat masked losses with a mask that differs between channels, and their all-false cases
    t = normals(rng, 2, 17, 19)
    p = t + noise(t.shape, 0.2)
    m = torch.from_numpy(rng.random((2, 3, 17, 19)) < 0.6)
    none = torch.zeros_like(m)
    d = dict(pred=p.numpy(), target=t.numpy(), mask=m.numpy())
    for key, fn, two in (("l1", ref.masked_l1_loss, True), ("mse", ref.masked_mse_loss, True), ("value", ref.masked_loss, False)):
        for tag, mm in (("", m), ("_empty", none)):
            a = p.clone().requires_grad_(True)
            # masked_loss writes into its argument: give it a copy inside the graph
            loss = fn(a, t, mm) if two else fn(a * 1.0, mm)
            if loss.requires_grad:
                loss.backward()
            a64 = p.double()
            loss64 = fn(a64, t.double(), mm) if two else fn(a64.clone(), mm)
            d[f"{key}{tag}"] = loss.detach().numpy()
            d[f"{key}{tag}_64"] = loss64.numpy()
            d[f"grad_{key}{tag}"] = (a.grad if a.grad is not None else torch.zeros_like(a)).numpy()
    path = os.path.join(OUT, "normal_masked.npz")
    np.savez_compressed(path, **d)
    print("masked:", {k: float(v) for k, v in d.items() if v.ndim == 0}, os.path.getsize(path), "B")

    # 7. make_valid_mask
    d = {}
    for i, (shape, pool) in enumerate((s, k) for s in ((1, 1, 8, 8), (2, 1, 37, 53), (1, 1, 5, 4)) for k in (4, 3)):
        B, _, H, W = shape
        m = torch.from_numpy((rng.random(shape) < 0.97).astype(np.float32))
        flat = m.view(-1)
        idx = rng.permutation(flat.numel())
        flat[idx[0]] = float("nan")
        flat[idx[1]] = 1.5                                   # 1 - m < 0: invalid only if it is the window's maximum
        flat[idx[2]] = 0.25
        m[:, :, H - 1, W // 2] = 0.0                         # invalid pixels in the last row and column: not pooled where
        m[:, :, H // 2, W - 1] = 0.0                         # H, W are no multiple of the pool
        valid = make_valid_mask(None, m.clone(), max_pool_size=pool)
        assert valid.shape == shape and valid.dtype == torch.bool
        assert torch.equal(valid, rs.valid_mask(m, pool)), (shape, pool)
        d[f"m{i}"], d[f"pool{i}"], d[f"valid{i}"] = m.numpy(), np.int64(pool), valid.numpy()
        print(f"validmask {shape} pool {pool}: {int(valid.sum())} of {valid.numel()} valid")
    d["count"] = np.int64(i + 1)
    path = os.path.join(OUT, "normal_validmask.npz")
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), "B")


if __name__ == "__main__":
    main()
