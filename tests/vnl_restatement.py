"""Torch restatement of the virtual normal loss (VNL_Loss of the reference's virtual_normal_loss.py), written from its
description in include/dptx.h; no reference code is imported.

forward(): every fp32 step as its own tensor op, i.e. rounded on its own, in the order csrc/vnl_loss.hip uses; returns the
per-triple keep flags, normals and losses, K, the cut, the loss, which triples are averaged under the stable-sort tie rule,
and the margins the GPU tests exempt (borderline mask decisions, kinks of |.|).
plain_loss(): the same function in differentiable torch ops on FIXED masks (for fp64 autograd).
"""
import numpy as np
import torch

DELTA_COS, DELTA_DIFF, ENERGY_EPS, ZERO_FILL, NORM_FILL = 0.867, 0.005, 1e-8, 0.0001, 0.01
ULP2 = 2.0 ** -22   # 2 fp32 ulps, relative


def linear_indices(p123, W):
    """the dict of select_index() -> three int64 tensors [n] of linear pixel indices y * W + x"""
    return tuple(torch.as_tensor(np.asarray(p123[f"p{j}_y"]).astype(np.int64) * W + np.asarray(p123[f"p{j}_x"]).astype(np.int64))
                 for j in (1, 2, 3))


def _points(depth, p, fx, fy):
    """depth [B,H,W] -> [3 coordinates][3 points] of [B,n] tensors: ((u - W//2) |d| / fx, (v - H//2) |d| / fy, d)"""
    B, H, W = depth.shape
    dt = depth.dtype
    flat = depth.reshape(B, H * W)
    fxt, fyt = torch.tensor(fx, dtype=dt), torch.tensor(fy, dtype=dt)
    P = [[None] * 3 for _ in range(3)]
    for j in range(3):
        d = flat[:, p[j]]
        u = (p[j] % W - W // 2).to(dt)
        v = (torch.div(p[j], W, rounding_mode="floor") - H // 2).to(dt)
        P[0][j] = _div(u * d.abs(), fxt)
        P[1][j] = _div(v * d.abs(), fyt)
        P[2][j] = d
    return P


def _sum3(a, b, c):
    return (a + b) + c


def _sqrt(x):
    """correctly rounded in the dtype of x, as the kernel's sqrtf is (torch's CPU sqrt of fp32 tensors is not: it differs
    from the IEEE result in the last bit of some values); fp64 sqrt rounded once more to fp32 is the IEEE fp32 result"""
    return torch.sqrt(x.double()).to(x.dtype) if x.dtype == torch.float32 else torch.sqrt(x)


def _div(a, b):
    """correctly rounded quotient in the dtype of a (fp64 quotient rounded once more to fp32 is the IEEE fp32 result)"""
    return (a.double() / b.double()).to(a.dtype) if a.dtype == torch.float32 else a / b


def _normal(P, zero=None):
    """cross(P2 - P1, P3 - P1), its norm with exact zeros replaced by 0.01 -> unit normal [3] of [B,n], zero flags.
    zero given (plain_loss): the replacement is taken from it, and nothing flows through a replaced norm."""
    a = [P[c][1] - P[c][0] for c in range(3)]
    b = [P[c][2] - P[c][0] for c in range(3)]
    N = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    sq = _sum3(N[0] * N[0], N[1] * N[1], N[2] * N[2])
    if zero is None:
        s = _sqrt(sq)
        zero = s == 0
        s = torch.where(zero, s + torch.tensor(NORM_FILL, dtype=s.dtype), s)
    else:
        s = torch.where(zero, torch.full_like(sq, NORM_FILL), torch.sqrt(torch.where(zero, torch.ones_like(sq), sq)))
    return [_div(N[c], s) for c in range(3)], zero


def _ulp(x):
    return float(np.spacing(np.float32(x)))


def forward(first, second, p, fx, fy, delta_z=0.0001, select=True, keep_on_borderline=None):
    """first, second [B,H,W] fp32 (CPU); p: three int64 tensors [n].  -> dict.  keep_on_borderline ([B,n] bool): the keep
    flags to adopt on the borderline triples (a mask comparison decided by less than rounding), so that K, the cut and the
    loss can be compared with an implementation that decided those the other way."""
    assert first.dtype == torch.float32 and second.dtype == torch.float32
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    B = first.shape[0]
    n = p[0].numel()
    P, Q = _points(first, p, fx, fy), _points(second, p, fx, fy)
    # the mask, on the first argument
    df = [[P[c][1] - P[c][0], P[c][2] - P[c][0], P[c][2] - P[c][1]] for c in range(3)]
    q = [_sqrt(_sum3(df[0][i] * df[0][i], df[1][i] * df[1][i], df[2][i] * df[2][i])) for i in range(3)]
    cnt = torch.zeros(B, n, dtype=torch.int64)
    border = torch.zeros(B, n, dtype=torch.bool)
    cos = f32(DELTA_COS)
    for i in range(3):
        for j in range(3):
            en = _sum3(df[0][i] * df[0][j], df[1][i] * df[1][j], df[2][i] * df[2][j])
            E = _div(en, q[i] * q[j] + f32(ENERGY_EPS))
            cnt += ((E > cos) | (E < -cos)).long()
            border |= (E.abs().double() - float(cos)).abs() <= 2.0 ** -20 * float(cos)
    collinear = cnt > 3
    dz = f32(delta_z)
    pad = (P[2][0] > dz) & (P[2][1] > dz) & (P[2][2] > dz)
    for j in range(3):
        border |= (P[2][j].double() - float(dz)).abs() <= _ulp(dz)
    dd = f32(DELTA_DIFF)
    near = []
    for c in range(3):
        near.append((df[c][0].abs() < dd) | (df[c][1].abs() < dd) | (df[c][2].abs() < dd))
        for i in range(3):
            border |= (df[c][i].abs().double() - float(dd)).abs() <= _ulp(dd)
    keep = pad & ~((near[0] & near[1] & near[2]) | collinear)
    if keep_on_borderline is not None:
        keep = torch.where(border, keep_on_borderline, keep)
    # z == 0 of point j of the second argument overwrites coordinate row j
    ow = [Q[2][j] == 0 for j in range(3)]
    same = (P[2][0] == Q[2][0]) & (P[2][1] == Q[2][1]) & (P[2][2] == Q[2][2])   # the same three depths: n_first == n_second
    Q = [[torch.where(ow[c], f32(ZERO_FILL), Q[c][j]) for j in range(3)] for c in range(3)]
    ng, z1 = _normal(P)
    nd, z2 = _normal(Q)
    diff = [ng[c] - nd[c] for c in range(3)]
    loss = _sum3(diff[0].abs(), diff[1].abs(), diff[2].abs())
    kink = torch.zeros(B, n, dtype=torch.bool)
    for c in range(3):
        kink |= (diff[c].abs() <= ULP2 * torch.maximum(ng[c].abs(), nd[c].abs())) & ~((ng[c] == 0) & (nd[c] == 0)) & ~same
    # the cut: stable ascending sort of the kept losses in (image, triple) order
    flat_keep = keep.reshape(-1)
    kept_idx = flat_keep.nonzero()[:, 0]
    K = int(kept_idx.numel())
    rank = int(K * 0.25) if select else 0
    vals = loss.reshape(-1)[kept_idx]
    order = torch.sort(vals, stable=True).indices
    active = torch.zeros(B * n, dtype=torch.bool)
    active[kept_idx[order[rank:]]] = True
    cut = float(vals[order[rank]]) if K > 0 else float("nan")
    total = loss.reshape(-1)[active].double().sum()
    count = K - rank
    value = (total / count).float() if count > 0 else torch.tensor(float("nan"))
    return dict(keep=keep, loss=torch.where(keep, loss, torch.zeros_like(loss)), normal_first=torch.stack(ng, -1),
                normal_second=torch.stack(nd, -1), K=K, rank=rank, cut=cut, active=active.reshape(B, n), value=value, count=count,
                borderline=border, kink=kink, zero_first=z1, zero_second=z2, overwritten=torch.stack(ow, -1))


def plain_loss(first, second, p, fx, fy, fixed):
    """The loss as differentiable torch ops in the dtype of the inputs, on the fixed decisions of forward() (`fixed`: its
    result): which triples are averaged, which rows were overwritten, which norms were replaced."""
    P, Q = _points(first, p, fx, fy), _points(second, p, fx, fy)
    ow = fixed["overwritten"]
    Q = [[torch.where(ow[..., c], torch.full_like(Q[c][j], ZERO_FILL), Q[c][j]) for j in range(3)] for c in range(3)]
    ng, _ = _normal(P, fixed["zero_first"])
    nd, _ = _normal(Q, fixed["zero_second"])
    loss = _sum3((ng[0] - nd[0]).abs(), (ng[1] - nd[1]).abs(), (ng[2] - nd[2]).abs())
    return torch.where(fixed["active"], loss, torch.zeros_like(loss)).sum() / fixed["count"]


def fp64_gradients(first, second, p, fx, fy, fixed):
    """d plain_loss / d (first, second) by fp64 autograd, [B,H,W] each (zeros when nothing is averaged)"""
    a = first.double().clone().requires_grad_(True)
    b = second.double().clone().requires_grad_(True)
    if fixed["count"] <= 0:
        return torch.zeros_like(a), torch.zeros_like(b)
    plain_loss(a, b, p, fx, fy, fixed).backward()
    return a.grad, b.grad


def kink_pixels(p, fixed, shape):
    """[B,H,W] bool: pixels touched by an averaged triple that has a component of n_first - n_second at the kink of |.|"""
    B, H, W = shape
    out = torch.zeros(B, H * W, dtype=torch.bool)
    k = fixed["kink"] & fixed["active"]
    for j in range(3):
        idx = p[j][None].expand(B, -1)
        out |= torch.zeros(B, H * W, dtype=torch.int32).scatter_add_(1, idx, k.int()) > 0
    return out.reshape(B, H, W)
