"""MiDaS loss on the GPU (omnidata_amd/midas_loss.py, csrc/midas_loss.hip) against CPU torch.nanmedian, the restatement
(tests/midas_restatement.py) and the reference's goldens (tools/make_midas_golden.py).  pytest -m gpu."""
import glob
import os

import numpy as np
import pytest
import torch

import midas_restatement as rs
from gpu_util import smooth, ulps
from omnidata_amd import midas_loss as ml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "midas_*.npz")))
LOSS_GOLDEN = [p for p in GOLDEN if not p.endswith("_parts.npz")]
ULP2 = 2.0 ** -22   # 2 fp32 ulps, relative


def values(kind, B, H, W, gen):
    if kind == "random":
        return torch.rand(B, H, W, generator=gen) * 5 + 0.01
    if kind == "ties":
        return torch.randint(0, 7, (B, H, W), generator=gen).float() * 0.25 + 0.5
    if kind == "signed":
        d = torch.randn(B, H, W, generator=gen)
        d.view(B, -1)[:, ::7] = 0.0
        d.view(B, -1)[:, 3::11] = -0.0
        return d
    if kind == "plateau":  # 16-bit decoded depth, half of the image at the far value 65535
        v = (smooth(gen, B, H, W, 200.0, 9000.0)[:, 0] / 32).round() * 32
        v.view(B, -1)[:, : (H * W) // 2] = 65535.0
        return (v / 65535.0) / torch.tensor(8000.0 / 65535.0)
    raise ValueError(kind)


def make_mask(frac, B, H, W, gen):
    if frac == "one":
        m = torch.zeros(B, H, W, dtype=torch.bool)
        for b in range(B):
            m.view(B, -1)[b, int(torch.randint(0, H * W, (1,), generator=gen))] = True
        return m
    return torch.rand(B, H, W, generator=gen) < frac


def case(B, H, W, seed, frac=0.8, kind="pair"):
    """pred, target [B,1,H,W] fp32 and mask (CPU): a target depth, a prediction that is an affine map of it plus a smooth
    field and noise"""
    gen = torch.Generator().manual_seed(seed)
    t = smooth(gen, B, H, W, 0.5, 6.0)[:, 0]
    p = 0.7 * t + 0.3 + 0.5 * smooth(gen, B, H, W, 0.0, 1.0)[:, 0] + 0.02 * torch.randn(B, H, W, generator=gen)
    if kind == "ties":
        p, t = (p * 4).round() / 4, (t * 2).round() / 2
    return p[:, None].contiguous(), t[:, None].contiguous(), make_mask(frac, B, H, W, gen)[:, None]


@pytest.mark.parametrize("shape", [(2, 384, 384), (3, 37, 53), (1, 1, 4097), (4, 512, 640)])
@pytest.mark.parametrize("kind", ["random", "ties", "signed", "plateau"])
@pytest.mark.parametrize("frac", [1.0, 0.5, 0.01, "one", 0.0])
def test_medians_equal_cpu_nanmedian(shape, kind, frac):
    B, H, W = shape
    gen = torch.Generator().manual_seed(B * 7 + H + W + len(kind) + (0 if frac == "one" else int(1000 * frac)))
    p, t = values(kind, B, H, W, gen), values(kind, B, H, W, gen)
    m = make_mask(frac, B, H, W, gen)
    st = ml.alignment_stats(p[:, None].cuda(), t[:, None].cuda(), m[:, None].cuda())
    for x, key in ((p, "t_p"), (t, "t_g")):
        want = x.masked_fill(~m, float("nan")).view(B, -1).nanmedian(-1).values
        want = torch.where(torch.isnan(want), torch.zeros_like(want), want)
        assert torch.equal(st[key].cpu(), want), (key, st[key], want)
    _, med = rs.medians(p.view(B, -1), m.view(B, -1))
    assert torch.equal(st["argmedian"].cpu(), med)
    assert torch.equal(st["n"].cpu(), m.view(B, -1).sum(1))


FWD = [  # B, H, W, terms, scales, image_based, alpha, frac
    (3, 48, 64, rs.ALL, 4, True, 0.1, 0.8),
    (3, 48, 64, rs.ALL, 4, False, 0.5, 0.8),
    (2, 37, 53, rs.ALL, 1, True, 0.5, 0.8),
    (2, 37, 53, rs.ALL, 2, False, 0.1, 0.5),
    (2, 40, 33, rs.ALL, 3, True, 0.1, 1.0),
    (2, 3, 5, rs.ALL, 4, True, 0.1, 1.0),        # H, W < 2^(scales-1)
    (3, 1, 37, rs.ALL, 4, False, 0.1, 0.8),
    (32, 384, 384, rs.ALL, 4, True, 0.1, 0.8),
    (3, 48, 64, rs.SSI, 1, True, 0.1, 0.8),
    (3, 48, 64, rs.GRAD, 4, False, 0.1, 0.8),
    (3, 48, 64, rs.GRAD, 3, True, 0.1, 0.8),
]


def run_loss(p, t, m, terms, scales, image_based, alpha, grad_losses=(1.0, 0.0, 0.0)):
    """the public callable for `terms` on the GPU -> (losses [3] as the kernel wrote them, grad [B,H,W] or None)"""
    pc = p.cuda().requires_grad_(grad_losses is not None)
    tc, mc = t.cuda(), m.cuda()
    red = "image-based" if image_based else "batch-based"
    if terms == rs.ALL:
        total, ssi, reg = ml.MidasLoss(alpha=alpha, scales=scales, reduction=red)(pc, tc, mc)
        outs = [total, ssi, reg]
    elif terms == rs.SSI:
        ssi = ml.SSIMAE()(pc, tc, mc)
        outs = [ssi, ssi, torch.zeros((), device="cuda")]
    else:
        reg = ml.GradientMatchingTerm(scales=scales, reduction=red)(pc[:, 0], tc[:, 0], mc[:, 0])
        outs = [reg, torch.zeros((), device="cuda"), reg]
    grad = None
    if grad_losses is not None:
        sel = [outs[0], outs[1], outs[2]] if terms == rs.ALL else [outs[1] if terms == rs.SSI else outs[2]]
        w = list(grad_losses) if terms == rs.ALL else [1.0]
        sum(wi * o for wi, o in zip(w, sel)).backward()
        grad = pc.grad[:, 0].cpu()
    return torch.stack([o.detach() for o in outs]).cpu(), grad


@pytest.mark.parametrize("c", FWD, ids=[f"B{c[0]}_{c[1]}x{c[2]}_t{c[3]}_s{c[4]}_{'img' if c[5] else 'bat'}_a{c[6]}" for c in FWD])
def test_forward_and_gradient_vs_restatement(c):
    B, H, W, terms, scales, image_based, alpha, frac = c
    p, t, m = case(B, H, W, seed=B * 31 + H + W + terms, frac=frac)
    gl = (1.0, 0.25, 0.5) if terms == rs.ALL else ((0.0, 1.0, 0.0) if terms == rs.SSI else (0.0, 0.0, 1.0))
    got, grad = run_loss(p, t, m, terms, scales, image_based, alpha, gl)
    ref = rs.forward(p[:, 0], t[:, 0], m[:, 0], terms, scales, image_based, alpha, grad_losses=gl, kink_rel=ULP2)
    want = ref["losses"].float()
    if terms == rs.SSI:
        want = torch.stack([want[1], want[1], torch.zeros(())])
    if terms == rs.GRAD:
        want = torch.stack([want[2], torch.zeros(()), want[2]])
    assert ulps(got, want).max() <= 2, (got, want)
    # gradient: elementwise within 1e-6 max|g|; pixels whose kink argument is within 2 ulps of 0 are exempt (counted)
    exempt = torch.zeros_like(m[:, 0])
    for key in ("ssi_kink", "reg_kink"):
        if key in ref:
            exempt |= ref[key]
    d = (grad.double() - ref["grad"]).abs()
    gmax = ref["grad"].abs().max().item()
    print(f"gradient: max|d| {d.max().item():.3e} of max|g| {gmax:.3e}, {int(exempt.sum())} kink exemptions")
    assert d[~exempt].max().item() <= 1e-6 * gmax


def test_alignment_outputs_vs_restatement():
    p, t, m = case(3, 45, 61, seed=5)
    st = ml.alignment_stats(p.cuda(), t.cuda(), m.cuda())
    ref = rs.forward(p[:, 0], t[:, 0], m[:, 0], rs.ALL)
    for k in ("t_p", "t_g", "s_p", "s_g", "scale", "shift"):
        assert ulps(st[k], ref[k]).max() <= (0 if k in ("t_p", "t_g") else 1), (k, st[k], ref[k])
    pa, ta = ml.masked_shift_and_scale(p.cuda(), t.cuda(), m.cuda())
    assert ulps(pa[:, 0], ref["pred_aligned"]).max() <= 1 and ulps(ta[:, 0], ref["target_aligned"]).max() <= 1
    sc, sh = ml.compute_scale_and_shift(p[:, 0].cuda(), t[:, 0].cuda(), m[:, 0].cuda())
    raw = rs.forward(p[:, 0], t[:, 0], m[:, 0], rs.GRAD | rs.ALIGN)
    assert ulps(sc, raw["scale"]).max() <= 1 and ulps(sh, raw["shift"]).max() <= 1


@pytest.mark.parametrize("path", LOSS_GOLDEN, ids=[os.path.basename(p)[6:-4] for p in LOSS_GOLDEN])
def test_reference_goldens(path):
    z = np.load(path)
    g = {k: torch.from_numpy(z[k]) for k in z.files}
    red = "image-based" if int(g["image_based"]) else "batch-based"
    pc = g["pred"].cuda().requires_grad_(True)
    total, ssi, reg = ml.MidasLoss(alpha=float(g["alpha"]), scales=int(g["scales"]), reduction=red)(pc, g["target"].cuda(),
                                                                                                   g["mask"].cuda())
    total.backward()
    got = torch.stack([total.detach(), ssi.detach(), reg.detach()]).cpu().double()
    want = g["losses"].double()
    assert ((got - want).abs() <= 1e-5 * want.abs()).all(), (got, want)
    out = rs.forward(g["pred"][:, 0], g["target"][:, 0], g["mask"][:, 0], rs.ALL, int(g["scales"]), bool(g["image_based"]),
                     float(g["alpha"]))
    rs.assert_grad_matches_reference(pc.grad[:, 0].cpu(), g["grad"][:, 0], g["pred"][:, 0], g["mask"][:, 0], out)


def test_reference_golden_parts():
    z = np.load(os.path.join(ROOT, "tests", "golden", "midas_parts.npz"))
    g = {k: torch.from_numpy(z[k]).cuda() for k in z.files}
    assert abs(ml.SSIMAE()(g["pred"], g["target"], g["mask"]).item() - g["ssi"].item()) <= 1e-5 * g["ssi"].item()
    pa, ta = ml.masked_shift_and_scale(g["pred"], g["target"], g["mask"])
    assert (pa - g["pred_aligned"]).abs().max() <= 1e-5 * g["pred_aligned"].abs().max()
    assert (ta - g["target_aligned"]).abs().max() <= 1e-5 * g["target_aligned"].abs().max()
    p, t, m = g["pred"][:, 0], g["target"][:, 0], g["mask"][:, 0]
    for red, s, key in (("batch-based", 4, "gm_batch_s4"), ("image-based", 3, "gm_image_s3")):
        v = ml.GradientMatchingTerm(scales=s, reduction=red)(p, t, m).item()
        assert abs(v - g[key].item()) <= 1e-5 * abs(g[key].item())
    sc, sh = ml.compute_scale_and_shift(p, t, m)
    md, pd = m.double(), p.double()   # bound of tests/test_midas_host.py: the reference's fp32 sums through the 2x2 solve
    a00, a01, n = (md * pd * pd).sum((1, 2)), (md * pd).sum((1, 2)), md.sum((1, 2))
    bound = n * 2.0 ** -24 * a00 * n / (a00 * n - a01 * a01)
    assert ((sc.double() - g["scale"].double()).abs() <= bound * g["scale"].double().abs()).all()
    assert ((sh.double() - g["shift"].double()).abs() <= bound * g["shift"].double().abs()).all()


def test_edge_cases():
    p, t, m = case(2, 24, 32, seed=3)
    # the whole batch masked: (nan, nan, 0), and no gradient
    got, grad = run_loss(p, t, torch.zeros_like(m), rs.ALL, 4, True, 0.1)
    assert torch.isnan(got[0]) and torch.isnan(got[1]) and got[2] == 0
    assert (grad == 0).all()
    # one valid pixel per image: (0, 0, 0)
    one = torch.zeros_like(m)
    one[0, 0, 3, 4] = one[1, 0, 20, 30] = True
    got, grad = run_loss(p, t, one, rs.ALL, 4, True, 0.1)
    assert (got == 0).all()
    # one image fully masked in the batch: finite, as the restatement
    m2 = m.clone()
    m2[1] = False
    got, grad = run_loss(p, t, m2, rs.ALL, 4, True, 0.1)
    ref = rs.forward(p[:, 0], t[:, 0], m2[:, 0], rs.ALL, grad_losses=(1.0, 0.0, 0.0))
    assert ulps(got, ref["losses"]).max() <= 2 and torch.isfinite(got).all()
    assert (grad.double() - ref["grad"]).abs().max() <= 1e-6 * ref["grad"].abs().max()
    # NaN in invalid prediction pixels: ssi finite, reg and total NaN (0 * NaN in the multiplicative masks)
    pn = p.clone()
    pn[~m] = float("nan")
    got, _ = run_loss(pn, t, m, rs.ALL, 4, True, 0.1, grad_losses=None)
    assert torch.isfinite(got[1]) and torch.isnan(got[0]) and torch.isnan(got[2])
    # constant prediction on the mask: det = 0 exactly, scale = shift = 0 (the restatement; the reference differs here)
    pc = torch.full_like(p, 2.5)
    got, grad = run_loss(pc, t, m, rs.ALL, 4, True, 0.1)
    ref = rs.forward(pc[:, 0], t[:, 0], m[:, 0], rs.ALL, grad_losses=(1.0, 0.0, 0.0))
    assert not ref["det_ok"].any()
    assert ulps(got, ref["losses"]).max() <= 2
    assert (grad.double() - ref["grad"]).abs().max() <= 1e-6 * ref["grad"].abs().max()


def test_ties_gradient_outside_and_sum_over_tie_set():
    p, t, m = case(2, 40, 48, seed=9, kind="ties")
    got, grad = run_loss(p, t, m, rs.ALL, 4, True, 0.1)
    ref = rs.forward(p[:, 0], t[:, 0], m[:, 0], rs.ALL, grad_losses=(1.0, 0.0, 0.0))
    assert ulps(got, ref["losses"]).max() <= 2
    gmax = ref["grad"].abs().max().item()
    for b in range(2):
        ties = m[b, 0] & (p[b, 0] == ref["t_p"][b])
        assert ties.sum() > 10
        d = (grad[b].double() - ref["grad"][b]).abs()
        assert d[~ties].max() <= 1e-6 * gmax
        assert abs(grad[b][ties].double().sum() - ref["grad"][b][ties].sum()) <= 1e-6 * gmax * int(ties.sum())


def test_two_losses_summed_before_one_backward():
    """The coefficient record of each call belongs to that call: a second forward on the same shape (same cached workspace)
    does not disturb the first one's backward."""
    (p1, t1, m1), (p2, t2, m2) = case(2, 40, 48, seed=1), case(2, 40, 48, seed=2)
    a = torch.cat([p1, p2], 1).cuda().requires_grad_(True)
    loss = ml.MidasLoss()
    l1 = loss(a[:, :1], t1.cuda(), m1.cuda())[0]
    l2 = loss(a[:, 1:], t2.cuda(), m2.cuda())[0]
    (l1 + 2.0 * l2).backward()
    r1 = rs.forward(p1[:, 0], t1[:, 0], m1[:, 0], grad_losses=(1.0, 0.0, 0.0))["grad"]
    r2 = rs.forward(p2[:, 0], t2[:, 0], m2[:, 0], grad_losses=(2.0, 0.0, 0.0))["grad"]
    g = a.grad.cpu().double()
    assert (g[:, 0] - r1).abs().max() <= 1e-6 * r1.abs().max()
    assert (g[:, 1] - r2).abs().max() <= 1e-6 * r2.abs().max()


def test_fp16_prediction_gradient_comes_back_in_fp16():
    p, t, m = case(2, 32, 40, seed=4)
    ph = p.half().cuda().requires_grad_(True)
    ml.MidasLoss()(ph, t.cuda(), m.cuda())[0].backward()
    assert ph.grad.dtype == torch.float16
    ref = rs.forward(ph.detach().float().cpu()[:, 0], t[:, 0], m[:, 0], grad_losses=(1.0, 0.0, 0.0))["grad"]
    assert (ph.grad.float().cpu()[:, 0].double() - ref).abs().max() <= 2e-3 * ref.abs().max()  # one fp16 rounding


def test_input_contract():
    p, t, m = (x.cuda() for x in case(2, 16, 16, seed=6))
    loss = ml.MidasLoss()
    with pytest.raises(ValueError):
        loss(p.cpu(), t.cpu(), m.cpu())
    with pytest.raises(ValueError):
        loss(p, t[:, :, :8], m)
    with pytest.raises(ValueError):
        loss(p[:, 0], t[:, 0], m[:, 0])
    with pytest.raises(ValueError):
        loss(p, t, m.float())
    with pytest.raises(ValueError):
        loss(p.double(), t.double(), m)
    with pytest.raises(ValueError):
        loss(p, t.clone().requires_grad_(True), m)
    for alpha in (0.0, -0.1):
        with pytest.raises(ValueError):
            ml.MidasLoss(alpha=alpha)(p, t, m)
    with pytest.raises(ValueError):
        ml.compute_scale_and_shift(p[:, 0].clone().requires_grad_(True), t[:, 0], m[:, 0])
    with pytest.raises(ValueError):
        ml.masked_shift_and_scale(p.clone().requires_grad_(True), t, m)
    with pytest.raises(ValueError):
        ml.GradientMatchingTerm()(p, t, m)


def test_repeat_bitwise_and_batch_invariance():
    p, t, m = case(7, 64, 80, seed=8)
    runs = []
    for _ in range(2):
        pc = p.cuda().requires_grad_(True)
        out = ml.MidasLoss()(pc, t.cuda(), m.cuda())
        out[0].backward()
        runs.append((torch.stack([o.detach() for o in out]).cpu(), pc.grad.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    full = ml.alignment_stats(p.cuda(), t.cuda(), m.cuda())
    for b in (0, 3, 6):
        one = ml.alignment_stats(p[b:b + 1].cuda(), t[b:b + 1].cuda(), m[b:b + 1].cuda())
        for k, v in one.items():
            assert torch.equal(v.cpu(), full[k][b:b + 1].cpu()), (b, k)


def test_training_smoke():
    """A small conv net trained 50 Adam steps with MidasLoss: the loss falls to at most half its start, and the first step's
    parameter gradients equal those from the restatement's gradient within 1e-5 relative."""
    torch.manual_seed(0)
    p, t, m = case(4, 32, 32, seed=10)
    x = torch.cat([t, torch.rand_like(t)], 1).cuda()    # the net sees the target depth and noise
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 16, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(16, 1, 3, padding=1),
                              torch.nn.Softplus()).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=3e-3)
    loss = ml.MidasLoss()
    tc, mc = t.cuda(), m.cuda()
    first = None
    for step in range(50):
        opt.zero_grad()
        y = net(x)
        total = loss(y, tc, mc)[0]
        total.backward()
        if step == 0:
            first = total.item()
            ref = rs.forward(y.detach().cpu()[:, 0], t[:, 0], m[:, 0], grad_losses=(1.0, 0.0, 0.0))["grad"]
            got = [q.grad.clone() for q in net.parameters()]
            net.zero_grad()
            net(x).backward(ref[:, None].float().cuda())
            for a, b in zip(got, net.parameters()):
                assert (a - b.grad).abs().max() <= 1e-5 * b.grad.abs().max(), (a - b.grad).abs().max()
            for q, gq in zip(net.parameters(), got):
                q.grad = gq
        opt.step()
    assert total.item() <= 0.5 * first, (first, total.item())
