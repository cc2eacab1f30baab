"""Surface-normal loss on the GPU (omnidata_amd/normal_loss.py, csrc/normal_loss.hip) against the restatement
(tests/normal_restatement.py) and the reference's goldens (tools/make_normal_golden.py).  pytest -m gpu.

Bounds.  Losses: those of tests/test_normal_host.py (derived there; the reference's own fp32 losses meet them).  Per-pixel
terms: |cos - cos_64| <= 16 * 2^-24 (same derivation) and l1 within 2 fp32 ulps of the fp64 sum of the three |p - t|: each is
one rounding, their fp64 sum is exact, so the kernel rounds a value within 2^-24 relative of the exact one, which lands at
most one fp32 neighbour away.  Gradients: the scaled error e = max |g - g64| / S of normal_restatement.scaled_error against
fp64 autograd, at most 2 e_ref (the reference's own fp32 error, recorded in the golden) floored at 1e-6; inputs without a
golden use the floor.  No pixel is exempt anywhere.
"""
import ctypes

import numpy as np
import pytest
import torch

import normal_restatement as rs
from gpu_util import ulps
from omnidata_amd import _native
from omnidata_amd import normal_loss as nl
from test_normal_host import LOSS_CASES, U, case, load, within

pytestmark = pytest.mark.gpu
SYNTHETIC = {"131x97": (3, 131, 97, 0), "96x132": (2, 96, 132, 0), "1x1": (1, 1, 1, 0), "clamp_64x80": (2, 64, 80, rs.CLAMP_PRED)}
ALL_CASES = LOSS_CASES + tuple(SYNTHETIC)
_inputs = {}


def inputs(name):
    """-> pred, target [B,3,H,W] fp32, mask [B,H,W] bool (CPU), flags, l1_weight, golden or None; computed once"""
    if name not in _inputs:
        if name in LOSS_CASES:
            g = load(name)
            _inputs[name] = (*case(g), g)
        else:
            B, H, W, fl = SYNTHETIC[name]
            gen = torch.Generator().manual_seed(B * 1000 + H)
            n = torch.randn(B, 3, H, W, generator=gen)
            t = (0.5 * n / n.norm(dim=1, keepdim=True) + 0.5).float()
            p = t + (0.4 if fl else 0.15) * torch.randn(B, 3, H, W, generator=gen)
            if not fl:
                p = p.clamp(0, 1)
            m = torch.rand(B, H, W, generator=gen) < 0.8
            if H * W == 1:
                m[:] = True
            _inputs[name] = (p.contiguous(), t.contiguous(), m, fl | rs.L1 | rs.COS, 10.0, None)
    return _inputs[name]


_restated = {}


def restated(name, flags, grad_losses):
    key = (name, flags, grad_losses)
    if key not in _restated:
        p, t, m, _, w, _ = inputs(name)
        _restated[key] = rs.evaluate(p, t, m, flags, w, grad_losses)
    return _restated[key]


def fused(p, t, m, flags, w, grad_losses=None):
    """the fused kernel pair behind every public entry -> losses (3,) CPU, grad [B,3,H,W] CPU or None"""
    a = p.cuda().requires_grad_(grad_losses is not None)
    out = nl._NormalLossFn.apply(a, t.cuda(), m.cuda().view(torch.uint8), flags, w)
    if grad_losses is not None:
        (out * torch.tensor(grad_losses, device="cuda")).sum().backward()
    return out.detach().cpu(), (a.grad.cpu() if grad_losses is not None else None)


def module_for(flags, w):
    return nl.NormalLoss(l1_weight=w, clamp_pred=bool(flags & rs.CLAMP_PRED))


def check_gradient(name, g, flags, grad_losses, bound, what):
    p, t, m, _, w, _ = inputs(name)
    ref = restated(name, flags, grad_losses)
    if ref["N"] == 0:
        assert not g.any()
        return
    e = rs.scaled_error(g, ref["grad"], rs.gradient_scale(ref, flags, w, grad_losses))
    print(f"{name} {what}: scaled error {e:.3e} (bound {bound:.3e}), max|g| {float(ref['grad'].abs().max()):.3e}")
    assert e <= bound
    assert not g[~m.unsqueeze(1).expand_as(g)].any()


@pytest.mark.parametrize("name", ALL_CASES)
def test_pixels_vs_restatement(name):
    p, t, m, flags, w, _ = inputs(name)
    cos, l1 = module_for(flags, w).pixels(p.cuda(), t.cuda(), m.unsqueeze(1).cuda())
    cos, l1 = cos.cpu(), l1.cpu()
    ref = restated(name, flags, None)
    assert cos.shape == l1.shape == m.shape
    d = (cos.double() - ref["cos64"])[m].abs()
    dl = ulps(l1[m], ref["l1_64"][m].float())
    print(f"{name}: max |cos - cos64| {float(d.max()) / U if d.numel() else 0:.2f} * 2^-24 over {int(m.sum())} pixels, l1 max "
          f"{int(dl.max()) if dl.size else 0} ulps; against the fp32 restatement: {int((cos != ref['cos32']).sum())} cos differ")
    assert d.numel() == 0 or float(d.max()) <= 16 * U
    assert dl.size == 0 or dl.max() <= 2
    assert not cos[~m].any() and not l1[~m].any()


@pytest.mark.parametrize("terms", [rs.L1, rs.COS, rs.L1 | rs.COS], ids=["l1", "cos", "both"])
@pytest.mark.parametrize("name", ALL_CASES)
def test_losses_vs_golden_and_restatement(name, terms):
    p, t, m, flags, w, g = inputs(name)
    fl = (flags & rs.CLAMP_PRED) | terms
    got, _ = fused(p, t, m, fl, w)
    ref = restated(name, fl, None)
    print(f"{name} terms {terms}: {got.tolist()} restatement fp64 {ref['losses64'].tolist()} fp32 terms {ref['losses32'].tolist()}")
    assert within(got.numpy(), ref["losses64"].numpy(), w)
    if g is not None:
        want = g["losses64"].copy()
        if terms == rs.L1:
            want[0], want[2] = want[1], 0.0
        elif terms == rs.COS:
            want[0], want[1] = want[2], 0.0
        assert within(got.numpy(), want, w)
    if terms == rs.L1:
        assert got[2] == 0 and (torch.equal(got[0], got[1]) or (torch.isnan(got[0]) and torch.isnan(got[1])))
    elif terms == rs.COS:
        assert got[1] == 0 and (torch.equal(got[0], got[2]) or (torch.isnan(got[0]) and torch.isnan(got[2])))
    if ref["N"] == 0:
        present = [0] + ([1] if terms & rs.L1 else []) + ([2] if terms & rs.COS else [])
        assert all(torch.isnan(got[i]) for i in present)


@pytest.mark.parametrize("name", ALL_CASES)
def test_normal_loss_gradients_vs_fp64_autograd(name):
    p, t, m, flags, w, g = inputs(name)
    bound = max(2 * float(g["e_ref"]), 1e-6) if g is not None else 1e-6
    mod = module_for(flags, w)
    mc = m.unsqueeze(1).cuda()
    for what, gl, scale in (("normal_loss", (1.0, 0.0, 0.0), None), ("2 l1 - 3 cos", (0.0, 2.0, -3.0), None),
                            ("0.37 normal_loss", (0.37, 0.0, 0.0), 0.37)):
        a = p.cuda().requires_grad_(True)
        out = mod(a, t.cuda(), mc)
        assert sorted(out) == ["cos_loss", "l1_loss", "normal_loss"] and all(v.dim() == 0 for v in out.values())
        if what == "2 l1 - 3 cos":
            (2 * out["l1_loss"] - 3 * out["cos_loss"]).backward()
        else:
            ((scale or 1.0) * out["normal_loss"]).backward()
        check_gradient(name, a.grad.cpu(), flags, tuple(float(np.float32(v)) for v in gl), bound, what)
        if restated(name, flags, None)["N"] == 0:
            assert torch.isnan(out["normal_loss"])


@pytest.mark.parametrize("name", ALL_CASES)
def test_drop_in_cosine_and_l1_gradients(name):
    p, t, m, flags, w, g = inputs(name)
    clamp = flags & rs.CLAMP_PRED
    tc = t.cuda()
    # the cosine loss with a three-channel mask whose channels 1 and 2 are garbage: channel 0 is the one that counts
    a = p.cuda().requires_grad_(True)
    m3 = torch.stack([m, ~m, torch.zeros_like(m)], 1).cuda()
    cos = nl.masked_cosine_angular_loss(a.clamp(0, 1) if clamp else a, tc, m3)
    cos.backward()
    bound = max(2 * float(g["e_ref_cos"]), 1e-6) if g is not None else 1e-6
    check_gradient(name, a.grad.cpu(), clamp | rs.COS, (0.0, 0.0, 1.0), bound, "masked_cosine_angular_loss")
    ref = restated(name, clamp | rs.COS, None)
    assert within([cos.item(), 0.0, cos.item()], ref["losses64"].numpy(), w)
    # the l1 loss through the flat kernel, the mask repeated over the channels as train_normal.py does
    a = p.cuda().requires_grad_(True)
    l1 = nl.masked_l1_loss(a.clamp(0, 1) if clamp else a, tc, m.unsqueeze(1).cuda().repeat_interleave(3, 1))
    l1.backward()
    bound = max(2 * float(g["e_ref"]), 1e-6) if g is not None else 1e-6
    check_gradient(name, a.grad.cpu(), clamp | rs.L1, (0.0, 1.0, 0.0), bound, "masked_l1_loss")
    ref = restated(name, clamp | rs.L1, None)
    assert within([l1.item(), l1.item(), 0.0], ref["losses64"].numpy(), w)


def test_flat_masked_losses_vs_golden_and_restatement():
    """masked_l1_loss, masked_mse_loss and masked_loss with a mask that differs between channels.  Loss: at most two roundings
    per element (the difference, the square), an exact fp64 sum and one final rounding, 3 * 2^-24 relative.  Gradient: sign / N,
    2 (p - t) / N and 1 / N are evaluated in fp64 and rounded once, 2^-24 relative per element (2^-23 allowed)."""
    g = load("masked")
    pred, target, mask = (torch.from_numpy(g[k]) for k in ("pred", "target", "mask"))
    calls = (("l1", rs.MASKED_L1, lambda a, mm: nl.masked_l1_loss(a, target.cuda(), mm)),
             ("mse", rs.MASKED_MSE, lambda a, mm: nl.masked_mse_loss(a, target.cuda(), mm)),
             ("value", rs.MASKED_VALUE | rs.MASKED_EMPTY_ZERO, lambda a, mm: nl.masked_loss(a, mm)))
    for key, kind, fn in calls:
        _, l64, g64, N = rs.masked(pred, target, mask, kind, grad=True)
        a = pred.cuda().requires_grad_(True)
        before = a.detach().clone()
        loss = fn(a, mask.cuda())
        (1.5 * loss).backward()
        got = a.grad.cpu().double()
        rel = abs(loss.item() - float(g[f"{key}_64"])) / abs(float(g[f"{key}_64"]))
        print(f"{key}: loss {loss.item():.9g} (reference fp64 {float(g[f'{key}_64']):.9g}, rel {rel:.2e}), max rel gradient error "
              f"{float(((got - 1.5 * g64).abs() / (1.5 * g64).abs().clamp_min(1e-300))[g64 != 0].max()):.2e}")
        assert loss.dim() == 0 and rel <= 3 * U and abs(loss.item() - float(l64)) <= 3 * U * abs(float(l64))
        assert ((got - 1.5 * g64).abs() <= 2 * U * (1.5 * g64).abs()).all() and torch.equal(got != 0, g64 != 0)
        assert ((got - 1.5 * torch.from_numpy(g[f"grad_{key}"]).double()).abs() <= 8 * U * (1.5 * g64).abs()).all()
        assert torch.equal(a.detach(), before)                       # the argument is left as it is (masked_loss docstring)
        a = pred.cuda().requires_grad_(True)
        empty = fn(a, torch.zeros_like(mask).cuda())
        empty.backward()
        assert (torch.isnan(empty) if key != "value" else empty.item() == 0.0) and not a.grad.any()
    # an odd element count (the scalar path) and more than one block
    gen = torch.Generator().manual_seed(5)
    p, t = torch.randn(3, 5, 67, 101, generator=gen), torch.randn(3, 5, 67, 101, generator=gen)
    m = torch.rand(3, 5, 67, 101, generator=gen) < 0.5
    for kind, fn in ((rs.MASKED_L1, nl.masked_l1_loss), (rs.MASKED_MSE, nl.masked_mse_loss)):
        _, l64, g64, _ = rs.masked(p, t, m, kind, grad=True)
        a = p.cuda().requires_grad_(True)
        loss = fn(a, t.cuda(), m.cuda())
        loss.backward()
        assert abs(loss.item() - float(l64)) <= 3 * U * abs(float(l64))
        assert ((a.grad.cpu().double() - g64).abs() <= 2 * U * g64.abs()).all()


def test_half_precision_inputs_get_their_own_gradient_dtype():
    p, t, m, flags, w, _ = inputs("unit")
    for dt, tol in ((torch.float16, 2.0 ** -10), (torch.bfloat16, 2.0 ** -7)):
        a = p.to(dt).cuda().requires_grad_(True)
        out = nl.NormalLoss()(a, t.to(dt).cuda(), m.unsqueeze(1).cuda())
        out["normal_loss"].backward()
        assert a.grad.dtype == dt and out["normal_loss"].dtype == torch.float32
        ref = rs.evaluate(a.detach().float().cpu(), t.to(dt).float(), m, rs.L1 | rs.COS | rs.CLAMP_PRED, 10.0, (1.0, 0.0, 0.0))
        assert within(torch.stack([out["normal_loss"], out["l1_loss"], out["cos_loss"]]).detach().cpu().numpy(), ref["losses64"].numpy(), 10.0)
        assert ((a.grad.float().cpu().double() - ref["grad"]).abs() <= tol * ref["grad"].abs() + 2.0 ** -24).all()   # one rounding to dt (fp16: subnormal below 2^-14)
        b = p.to(dt).cuda().requires_grad_(True)
        nl.masked_l1_loss(b, t.to(dt).cuda(), m.unsqueeze(1).expand(-1, 3, -1, -1).cuda()).backward()
        assert b.grad.dtype == dt


def test_reference_equivalences():
    p, t, m, flags, w, _ = inputs("clamp")
    pc, tc, m1 = p.cuda(), t.cuda(), m.unsqueeze(1).cuda()
    # CLAMP_PRED equals clamping in torch first, bit for bit, gradient included
    a = pc.clone().requires_grad_(True)
    out_a = nl.NormalLoss(clamp_pred=True)(a, tc, m1)
    out_a["normal_loss"].backward()
    b = pc.clone().requires_grad_(True)
    out_b = nl.NormalLoss(clamp_pred=False)(torch.clamp(b, 0, 1), tc, m1)
    out_b["normal_loss"].backward()
    for k in out_a:
        assert torch.equal(out_a[k], out_b[k]), k
    assert torch.equal(a.grad, b.grad) and a.grad[(pc == 1) & m1].any() and not a.grad[(pc > 1) | (pc < 0)].any()
    # a [B,1,H,W] mask equals its repeat_interleave(3, 1)
    c = pc.clone().requires_grad_(True)
    out_c = nl.NormalLoss()(c, tc, m1.repeat_interleave(3, 1))
    out_c["normal_loss"].backward()
    assert all(torch.equal(out_a[k], out_c[k]) for k in out_a) and torch.equal(a.grad, c.grad)
    # NormalLoss equals the two functions called separately (train_normal.py:251-258)
    d = pc.clone().requires_grad_(True)
    dcl = torch.clamp(d, 0, 1)
    m3 = m1.repeat_interleave(3, 1)
    cos = nl.masked_cosine_angular_loss(dcl, tc, m3)
    l1 = nl.masked_l1_loss(dcl, tc, m3)
    assert torch.equal(cos, out_a["cos_loss"])                        # the same kernel, the same order of summation
    assert abs(l1.item() - out_a["l1_loss"].item()) <= 4 * U * l1.item()   # each within 2 * 2^-24 of the fp64 value
    gc, = torch.autograd.grad(cos, d, retain_graph=True)
    gl, = torch.autograd.grad(l1, d)
    assert ((a.grad - (gc + 10 * gl)).abs() <= 4 * U * (gc.abs() + 10 * gl.abs())).all()


def test_valid_mask_goldens_and_random_masks():
    v = load("validmask")
    for i in range(int(v["count"])):
        got = nl.make_valid_mask(torch.from_numpy(v[f"m{i}"]).cuda(), int(v[f"pool{i}"]))
        assert got.dtype == torch.bool and torch.equal(got.cpu(), torch.from_numpy(v[f"valid{i}"])), i
    gen = torch.Generator().manual_seed(3)
    for shape in ((3, 1, 37, 53), (1, 1, 4, 4), (2, 1, 64, 96), (1, 1, 130, 7)):
        for pool in (4, 3):
            m = (torch.rand(shape, generator=gen) < 0.97).float()
            m.view(-1)[torch.randperm(m.numel(), generator=gen)[:3]] = torch.tensor([float("nan"), 1.5, 0.25])
            got = nl.make_valid_mask(m.cuda(), pool)
            assert got.shape == shape and torch.equal(got.cpu(), rs.valid_mask(m, pool)), (shape, pool)
    m = (torch.rand(9, 12, generator=gen) < 0.9).float()
    want = rs.valid_mask(m.view(1, 1, 9, 12), 4)
    assert torch.equal(nl.make_valid_mask(m.cuda()).cpu(), want)                              # 2-D, the default pool
    assert torch.equal(nl.make_valid_mask(m.view(1, 9, 12).cuda()).cpu(), want)               # 3-D
    assert torch.equal(nl.make_valid_mask(m.half().cuda()).cpu(), want)


def _abi_run(p, t, m, flags, w, gl, stream=None):
    """the C ABI itself on buffers filled with 0xFF bytes -> losses, record, grad (CPU)"""
    from omnidata_amd.engine import load_library
    lib = load_library()
    B, _, H, W = p.shape
    nbytes = ctypes.c_int64()
    assert lib.dptx_normal_workspace_bytes(B, H, W, ctypes.byref(nbytes)) == 0
    ff = lambda n, dt: torch.full((n,), 255, dtype=torch.uint8, device="cuda").view(dt)   # noqa: E731
    ws, losses, record, grad = ff(nbytes.value, torch.uint8), ff(12, torch.float32), ff(32, torch.float64), ff(4 * p.numel(), torch.float32)
    glc = torch.tensor(gl, device="cuda")
    st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    assert lib.dptx_normal_loss(p.data_ptr(), t.data_ptr(), m.data_ptr(), B, H, W, flags, w, losses.data_ptr(), record.data_ptr(),
                                ws.data_ptr(), nbytes.value, st) == 0
    assert lib.dptx_normal_loss_backward(p.data_ptr(), t.data_ptr(), m.data_ptr(), B, H, W, flags, w, record.data_ptr(), glc.data_ptr(),
                                         grad.data_ptr(), st) == 0
    torch.cuda.synchronize()
    return losses.cpu(), record.cpu(), grad.view(p.shape).cpu()


@pytest.mark.parametrize("name", ["96x132", "131x97"])
def test_repeat_bitwise_poisoned_buffers_other_stream_and_alignment(name):
    p, t, m, flags, w, _ = inputs(name)
    gl = (1.0, 0.5, -2.0)
    first = fused(p, t, m, flags, w, gl)
    again = fused(p, t, m, flags, w, gl)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    for ws in _native._ws_cache.values():
        ws.fill_(255)
    poisoned = fused(p, t, m, flags, w, gl)
    assert torch.equal(first[0], poisoned[0]) and torch.equal(first[1], poisoned[1])
    pc, tc, mc = p.cuda(), t.cuda(), m.cuda().view(torch.uint8)
    losses, record, grad = _abi_run(pc, tc, mc, flags, w, gl)
    assert torch.equal(losses, first[0]) and torch.equal(grad, first[1]) and record[0].item() == float(m.sum())
    assert record.view(torch.uint8)[8 * nl.RECORD_DOUBLES:].eq(255).all()      # the record is the count alone
    # a non-default stream
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = fused(p, t, m, flags, w, gl)
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])
    # pointers that are not 16-byte aligned take the scalar path: the same units, so the same bits
    shifted = []
    for x, dt in ((pc, torch.float32), (tc, torch.float32), (mc, torch.uint8)):
        buf = torch.empty(x.numel() + 1, dtype=dt, device="cuda")
        buf[1:].copy_(x.reshape(-1))
        shifted.append(buf[1:].view(x.shape))
    assert shifted[0].data_ptr() % 16 != 0
    losses, _, grad = _abi_run(*shifted, flags, w, gl)
    assert torch.equal(losses, first[0]) and torch.equal(grad, first[1])


def test_two_losses_summed_before_one_backward():
    """The record belongs to the call: a second forward on the same shape (the same cached workspace) with another mask does
    not disturb the first one's backward."""
    p, t, m, flags, w, _ = inputs("96x132")
    m2 = ~m
    a = p.cuda().requires_grad_(True)
    mod = nl.NormalLoss(clamp_pred=False)
    l1 = mod(a, t.cuda(), m.unsqueeze(1).cuda())["normal_loss"]
    l2 = mod(a, t.cuda(), m2.unsqueeze(1).cuda())["normal_loss"]
    (l1 + 2.0 * l2).backward()
    g = a.grad.cpu()
    r1 = rs.evaluate(p, t, m, flags, w, (1.0, 0.0, 0.0))
    r2 = rs.evaluate(p, t, m2, flags, w, (2.0, 0.0, 0.0))
    m4, m24 = m.unsqueeze(1).expand_as(g), m2.unsqueeze(1).expand_as(g)
    assert rs.scaled_error(torch.where(m4, g, torch.zeros_like(g)), r1["grad"], rs.gradient_scale(r1, flags, w, (1.0, 0.0, 0.0))) <= 1e-6
    assert rs.scaled_error(torch.where(m24, g, torch.zeros_like(g)), r2["grad"], rs.gradient_scale(r2, flags, w, (2.0, 0.0, 0.0))) <= 1e-6


def test_input_contract():
    p, t, m, _, _, _ = inputs("unit")
    a, b, mm = p.cuda(), t.cuda(), m.unsqueeze(1).cuda()
    mod = nl.NormalLoss()
    assert mod(a, b, mm)["normal_loss"].dim() == 0
    other = "cuda:1" if torch.cuda.device_count() > 1 else None
    bad = [(a.cpu(), b.cpu(), mm.cpu()), (a, b, mm.cpu()), (a[0], b[0], mm[0]), (a[:, :2], b[:, :2], mm), (a, b[:, :, :8], mm),
           (a, b, mm[:, :, :8]), (a, b, mm.expand(-1, 2, -1, -1)), (a.double(), b.double(), mm), (a, b, mm.unsqueeze(1))]
    if other:
        bad.append((a, b.to(other), mm))
    for args in bad:
        with pytest.raises(ValueError):
            mod(*args)
        with pytest.raises(ValueError):
            nl.masked_cosine_angular_loss(*args)
    m3 = mm.expand(-1, 3, -1, -1)
    for args in ((a.cpu(), b.cpu(), m3.cpu()), (a, b[:, :, :8], m3), (a, b, mm), (a, b, m3.float()), (a.double(), b, m3)):
        with pytest.raises(ValueError):
            nl.masked_l1_loss(*args)
        with pytest.raises(ValueError):
            nl.masked_mse_loss(*args)
    with pytest.raises(ValueError):
        nl.masked_loss(a, mm)
    mf = m.float().cuda()
    for args in ((mf.cpu(),), (mf.view(2, 1, 1, *mf.shape[1:]),), (mf[0, :3], 4), (mf, 0), (m.cuda(),)):
        with pytest.raises(ValueError):
            nl.make_valid_mask(*args)
