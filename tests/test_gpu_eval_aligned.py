"""Scale-and-shift-aligned depth evaluation on the GPU (include/dptx.h dptx_eval_depth_aligned, omnidata_amd.gpu_metrics
aligned_depth_metrics): the coefficients are those of dptx_midas_stats bit for bit, fields 0-7 those of dptx_eval_depth on the
aligned tensor bit for bit, fields 8-14 those of tests/eval_aligned_restatement.py, and all of it the reference's numbers on
the goldens of tools/make_eval_aligned_golden.py.  pytest -m gpu.

Shapes (B, H, W): (2, 37, 53) scalar loads, two metric blocks per image; (3, 48, 64) 16-byte loads, three blocks; (2, 96, 130)
13 metric blocks and 4 blocks of the statistics per image.  Inputs: eval_aligned_restatement.inputs.

Measured on an MI355X (profiles/eval_aligned_parity.md has the table): see the figures each test prints."""
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch

import eval_aligned_restatement as rs
from gpu_util import ulps
from omnidata_amd import _native
from omnidata_amd import gpu_metrics as gm
from omnidata_amd import midas_loss as ml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "evalaligned_*.npz")))
SHAPES = ((2, 37, 53), (3, 48, 64), (2, 96, 130))
ALIGNS = ("lstsq", "median")
ULP2 = 2.0 ** -22   # 2 fp32 ulps, relative
EPS = np.float32(1e-6)
_cases = {}


def case(B, H, W, seed=11, **kw):
    """the shared inputs of one shape, on the device; computed once and never written to"""
    key = (B, H, W, seed, tuple(sorted(kw.items())))
    if key not in _cases:
        _cases[key] = tuple(x.cuda() for x in rs.inputs(seed, B, H, W, **kw))
    return _cases[key]


def bits(x):
    return x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def crit(got, want):
    """the project's metric criterion: |d| / max(1, |v|); NaN on both sides agrees (an unclamped aligned value below -1 / 64
    makes the reference's log terms NaN), NaN on one side is infinitely far"""
    got, want = got.double().cpu(), want.double().cpu()
    d = (got - want).abs() / want.abs().clamp(min=1.0)
    d = torch.where(torch.isnan(got) & torch.isnan(want), torch.zeros_like(d), d)
    return float(d.nan_to_num(nan=float("inf")).max())


def same_floats(a, b):
    """two dicts of floats with the same keys in the same order and the same bits (a NaN equals itself here)"""
    return list(a) == list(b) and np.array_equal(np.array(list(a.values()), dtype=np.float64).view(np.int64),
                                                 np.array(list(b.values()), dtype=np.float64).view(np.int64))


def run(p, t, m, align, clamp=True, min_depth=1e-3):
    """-> rows [B + 1, 15] fp64, coeffs [B, 2], aligned [B,1,H,W]"""
    return gm._aligned_rows(p, t, m, align, clamp, min_depth, True)


def device_stats(p, t, m):
    """the statistics of dptx_midas_stats in the restatement's form, and pred_aligned of masked_shift_and_scale"""
    a = ml._stats(p, t, m, 4, ml.ALIGN)[0]
    s, pa, _ = ml._stats(p, t, m, 4, ml.SSI, aligned=True)
    return {"t_p": s[:, 0], "t_g": s[:, 1], "s_p": s[:, 2], "s_g": s[:, 3], "scale": a[:, 5], "shift": a[:, 6]}, pa.view(p.shape)


def composed(p, align, st, pa, clamp):
    """the aligned tensor from torch fp32 ops, one rounding each, out of what dptx_midas_stats returns"""
    v = lambda x: x.view(-1, 1, 1, 1)
    if align == "lstsq":
        a = v(st["scale"]) * p
        a = a + v(st["shift"])
    else:
        a = pa * (v(st["s_g"]) + EPS)
        a = a + v(st["t_g"])
    return a.clamp(0, 1) if clamp else a


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_coefficients_are_those_of_midas_stats(shape, align):
    p, t, m = case(*shape)
    st, _ = device_stats(p, t, m)
    _, co, _ = run(p, t, m, align)
    want = rs.coeffs(align, {k: v.cpu() for k, v in st.items()})   # MEDIAN: two fp32 operations on the CPU, rounded as IEEE says
    assert same_bits(co.cpu(), want), (co, want)


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_fields_0_to_7_are_eval_depth_of_the_aligned_tensor(shape, align, clamp):
    p, t, m = case(*shape)
    st, pa = device_stats(p, t, m)
    comp = composed(p, align, st, pa, clamp)
    rows, _, al = run(p, t, m, align, clamp)
    assert same_bits(al, comp)
    B = shape[0]
    assert same_bits(rows[:B, :8], gm._rows("depth_zbuffer", comp, t, m, True))
    assert same_bits(rows[B:, :8], gm._rows("depth_zbuffer", comp, t, m, False))
    if clamp:
        assert float(al.min()) >= 0.0 and float(al.max()) <= 1.0


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_fields_8_to_14_match_the_restatement(shape, align):
    p, t, m = case(*shape)
    st, _ = device_stats(p, t, m)
    for clamp, md in ((True, 1e-3), (False, 0.25)):   # 0.25 floors a good part of both depths
        rows, _, _ = run(p, t, m, align, clamp, md)
        want = rs.rows(rs.aligned(p.cpu(), align, st, clamp), t, m, md)   # fp32 on the CPU: every operation IEEE-rounded
        assert torch.equal(rows[:, 12:].cpu(), want[:, 12:]), (rows[:, 12:], want[:, 12:])
        assert torch.equal(rows[:, 0].cpu(), want[:, 0])
        d = crit(rows[:, :12], want[:, :12])
        print(f"\n[aligned {shape} {align} clamp={clamp} min_depth={md}] fields 1-11 vs restatement: {d:.2e}; "
              f"delta1 {rows[-1, 12].item():.4f}")
        assert d < 1e-6


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[12:-4] for p in GOLDEN])
def test_reference_goldens(path):
    """Coefficients within 1 fp32 ulp of the reference's fp64 run (the bar of test_gpu_midas.py), rows within the 1e-6
    criterion of the reference's row.  MEDIAN: the statistics the call uses (those of dptx_midas_stats, which
    test_coefficients_are_those_of_midas_stats ties to it bit for bit) -- the medians 0 ulp, the deviations within 1 ulp --
    and the reported pair within 1 ulp of the pair formed from the reference's statistics."""
    z = np.load(path)
    g = {k: torch.from_numpy(z[k]) for k in z.files if z[k].dtype.kind in "fb"}
    keys = [str(k) for k in z["keys"]]
    p, t, m = g["pred"].cuda(), g["target"].cuda(), g["mask"].cuda()
    B = p.shape[0]
    for align in ALIGNS:
        rows, co, _ = run(p, t, m, align)
        co = co.cpu()
        if align == "lstsq":
            u = ulps(co, g["coeffs64"]).max()
            print(f"\n[{os.path.basename(path)}] lstsq coefficients: {u} ulp from the reference's fp64 run")
            assert u <= 1
        else:
            s64 = g["stats64"]
            st, _ = device_stats(p, t, m)
            us = {k: int(ulps(st[k], s64[:, j]).max()) for j, k in enumerate(("t_p", "t_g", "s_p", "s_g"))}
            want = rs.coeffs("median", {"t_p": s64[:, 0], "t_g": s64[:, 1], "s_p": s64[:, 2], "s_g": s64[:, 3]})
            up = int(ulps(co, want).max())
            print(f"[{os.path.basename(path)}] median statistics: {us} ulp, reported pair {up} ulp from the reference's fp64 run")
            assert us["t_p"] == 0 and us["t_g"] == 0 and us["s_p"] <= 1 and us["s_g"] <= 1
            assert up <= 1
        ref = torch.full((B + 1, 15), float("nan"), dtype=torch.float64)
        for k, name in enumerate(keys):
            ref[:B, rs.FIELDS.index(name)] = g[align + "_images"][:, k]
            ref[B, rs.FIELDS.index(name)] = g[align + "_batch"][k]
        have = ~torch.isnan(ref)
        assert have[:, 1:8].all()
        d = crit(rows.cpu()[have], ref[have])
        print(f"[{os.path.basename(path)}] {align} rows vs the reference's: {d:.2e}")
        assert d < 1e-6
        n = g["mask"].reshape(B, -1).sum(1).double()
        assert torch.equal(rows[:, 0].cpu(), torch.cat([n, n.sum()[None]]))


def test_planted_fit_is_recovered():
    p, t, m = case(3, 48, 64, seed=21, noise=0.0, field=0.0)
    rows, co, _ = run(p, t, m, "lstsq")
    co = co.double().cpu()
    rel = max(float((co[:, 0] - 1.7).abs().max()) / 1.7, float((co[:, 1] - 0.2).abs().max()) / 0.2)
    raw = gm.depth_metrics(p, t, m)["eval_L1"].item()
    fit = rows[-1, 1].item()
    print(f"\n[planted] scale, shift within {rel:.2e} of (1.7, 0.2); eval_L1 {raw:.3f} unaligned, {fit:.3e} aligned")
    assert rel <= ULP2
    assert fit <= 1e-3 * raw


@pytest.mark.parametrize("align", ALIGNS)
def test_edges(align):
    """Image 1 has an empty mask, image 2 a constant prediction, image 0 a target of 0 on valid pixels.  Rows with n > 0 are
    finite, with one exception that fields 0-7 inherit from the reference's formula bit for bit: rel_error divides by the
    target, so a valid pixel with target 0 makes it inf in its image's row and in the batch row.  Fields 8-14 floor both
    depths and stay finite."""
    p, t, m = (x.clone() for x in case(3, 37, 53))
    m[1] = False
    p[2] = 0.5   # sums of 0.5 and 0.25 are exact: det == 0 exactly
    t[0, 0, 5:9, 7:20] = 0.0
    m[0, 0, 5:9, 7:20] = True
    rows, co, al = run(p, t, m, align)
    rows, co = rows.cpu(), co.cpu()
    assert rows[1, 0] == 0 and torch.isnan(rows[1, 1:]).all()
    assert (rows[[0, 2, 3], 0] > 0).all()
    assert torch.isfinite(rows[[0, 2, 3], 8:]).all(), rows
    assert torch.isfinite(rows[2, :8]).all()
    finite = torch.isfinite(rows[[0, 3], :8])
    assert finite[:, [0, 1, 2, 3, 4, 5, 7]].all() and torch.isinf(rows[[0, 3], 6]).all(), rows
    assert torch.isfinite(al).all()
    if align == "lstsq":
        assert co[1].tolist() == [0.0, 0.0] and co[2].tolist() == [0.0, 0.0]
        assert float(al[1].abs().max()) == 0.0 and float(al[2].abs().max()) == 0.0
    else:   # s_p = 0: every pixel of the constant image goes to the target's median
        st, _ = device_stats(p, t, m)
        assert same_bits(al[2], st["t_g"][2].expand_as(al[2]).clamp(0, 1).contiguous())
    # the floor: image 0's abs_rel counts |a_e - 1e-3| / 1e-3 on the zero-target pixels, as the restatement does
    st, _ = device_stats(p, t, m)
    want = rs.rows(rs.aligned(p.cpu(), align, st, True), t, m)
    assert torch.equal(rows[[0, 2, 3], 12:], want[[0, 2, 3], 12:])
    assert crit(rows[[0, 2, 3], 8:12], want[[0, 2, 3], 8:12]) < 1e-6


@pytest.mark.parametrize("align", ALIGNS)
def test_non_finite_inputs_stay_in_their_image(align):
    p, t, m = (x.clone() for x in case(3, 48, 64))
    clean = run(p, t, m, align)[0]
    p[1, 0, 3, 5] = float("nan")
    p[1, 0, 9, 9] = float("inf")
    m[1, 0, 3, 5] = m[1, 0, 9, 9] = True
    rows, co, _ = run(p, t, m, align)
    assert same_bits(rows[[0, 2]], clean[[0, 2]]) and torch.isfinite(co[[0, 2]]).all()
    assert rows[1, 0] == int(m[1].sum()) and rows[3, 0] == int(m.sum())


@pytest.mark.parametrize("align", ALIGNS)
def test_bitwise_repeat_batch_independence_and_workspace(align):
    p, t, m = case(3, 48, 64)
    other = ALIGNS[1 - ALIGNS.index(align)]
    first = run(p, t, m, align)
    run(p, t, m, other)                                      # the same cached workspace, the other mode in between
    for ws in _native._ws_cache.values():                    # and whatever any call left behind, overwritten
        if ws.is_cuda:
            ws.fill_(0xFF)
    again = run(p, t, m, align)
    for a, b in zip(first, again):
        assert same_bits(a, b)
    for i in range(3):                                       # a per-image row alone: the same bits, in both of its rows
        rows, co, al = run(p[i:i + 1], t[i:i + 1], m[i:i + 1], align)
        assert same_bits(rows[0], first[0][i]) and same_bits(rows[1], first[0][i])
        assert same_bits(co[0], first[1][i]) and same_bits(al[0], first[2][i])


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("shape", [(3, 48, 64), (2, 37, 53)])
def test_bitwise_on_pointers_misaligned_by_4_bytes(shape, align):
    p, t, m = case(*shape)
    want = run(p, t, m, align)

    def shifted(x):
        buf = torch.empty(x.numel() + 4 // x.element_size(), dtype=x.dtype, device=x.device)
        y = buf[4 // x.element_size():].view(x.shape)
        y.copy_(x)
        assert y.data_ptr() % 16 == 4 and y.is_contiguous()
        return y
    got = run(shifted(p), shifted(t), shifted(m), align)
    for a, b in zip(want, got):
        assert same_bits(a, b)


@pytest.mark.parametrize("align", ALIGNS)
def test_bitwise_with_only_the_aligned_output_off_16_bytes(align):
    """Inputs on 16-byte boundaries, H*W % 4 == 0, but `aligned` moved by 4 bytes: the call must take the scalar path (a
    16-byte store there would be misaligned) and give the same bits.  Through the C ABI: the Python layer always allocates
    the output on a boundary."""
    from omnidata_amd.engine import _stream
    p, t, m = case(3, 48, 64)
    want = run(p, t, m, align)
    B, _, H, W = p.shape
    ws = _native.workspace("dptx_eval_aligned_workspace_bytes", p.device, (B, H, W), "shape")
    out = torch.empty(B + 1, 15, dtype=torch.float64, device=p.device)
    co = torch.empty(B, 2, device=p.device)
    buf = torch.full((p.numel() + 2,), float("nan"), device=p.device)
    al = buf[1:-1]
    assert al.data_ptr() % 16 == 4 and p.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0
    _native.call("dptx_eval_depth_aligned", p.data_ptr(), t.data_ptr(), m.view(torch.uint8).data_ptr(), B, H, W, gm._ALIGN[align],
                 gm.ALIGNED_CLAMP, 1e-3, out.data_ptr(), co.data_ptr(), al.data_ptr(), ws.data_ptr(), ws.numel(), _stream(p.device))
    assert same_bits(out, want[0]) and same_bits(co, want[1]) and same_bits(al.view(p.shape), want[2])
    assert torch.isnan(buf[0]) and torch.isnan(buf[-1])   # nothing written outside the output


def test_python_argument_contract():
    p, t, m = case(2, 37, 53)
    d = gm.aligned_depth_metrics(p, t, m)
    assert tuple(d) == gm.ALIGNED_DEPTH_FIELDS == rs.FIELDS and all(v.dtype == torch.float64 and v.is_cuda and v.dim() == 0 for v in d.values())
    d, co, al = gm.aligned_depth_metrics(p, t, m, align="median", per_image=True, return_coeffs=True, return_aligned=True)
    assert all(v.shape == (2,) for v in d.values()) and co.shape == (2, 2) and al.shape == p.shape
    al2, co2 = gm.align_depth(p, t, m, "median")
    assert same_bits(co, co2) and same_bits(al2.clamp(0, 1), al)
    half = gm.aligned_depth_metrics(p.half(), t.half(), m)      # fp16 inputs are widened, as elsewhere in the module
    assert torch.isfinite(half["abs_rel"])
    assert same_bits(gm.aligned_depth_metrics(p, t, m, min_depth=np.float32(1e-3))["abs_rel"], gm.aligned_depth_metrics(p, t, m)["abs_rel"])
    for bad in (dict(align="affine"), dict(align=None), dict(min_depth=0.0), dict(min_depth=float("nan")), dict(min_depth=-1.0),
                dict(min_depth=1e-50), dict(min_depth=1e39), dict(min_depth=None), dict(min_depth="1e-3x")):
        with pytest.raises(ValueError):
            gm.aligned_depth_metrics(p, t, m, **bad)
    with pytest.raises(ValueError):
        gm.aligned_depth_metrics(p.cpu(), t.cpu(), m.cpu())
    with pytest.raises(ValueError):
        gm.aligned_depth_metrics(p, t, m.float())
    with pytest.raises(ValueError):
        gm.aligned_depth_metrics(p.expand(-1, 3, -1, -1), t.expand(-1, 3, -1, -1), m)
    with pytest.raises(ValueError):
        gm.get_metrics(p.expand(-1, 3, -1, -1), t.expand(-1, 3, -1, -1), "normal", m, align="lstsq")
    with pytest.raises(ValueError):
        gm.MetricsAccumulator("normal", align="lstsq")
    with pytest.raises(ValueError):
        gm.MetricsAccumulator("depth_zbuffer", align="affine")


def test_get_metrics_without_align_is_unchanged_and_with_align_is_the_batch_row():
    p, t, m = case(2, 37, 53)
    row = gm._rows("depth_zbuffer", p, t, m, False)[0].cpu().tolist()
    before = dict(zip(gm.DEPTH_FIELDS[1:], row[1:]))   # the unaligned prediction dips below -1 / 64: log10 and si_log are NaN
    assert same_floats(gm.get_metrics(p, t, "depth_zbuffer", m), before)
    assert same_floats(gm.get_metrics(p, t, "depth_zbuffer", m, align=None), before)
    rows = run(p, t, m, "lstsq")[0]
    got = gm.get_metrics(p, t, "depth_zbuffer", m, align="lstsq")
    assert same_floats(got, dict(zip(gm.ALIGNED_DEPTH_FIELDS[1:], rows[-1, 1:].cpu().tolist())))
    assert gm.get_metrics(p, t, "depth_zbuffer", torch.zeros_like(m), align="median") is None
    loose = gm.get_metrics(p, t, "depth_zbuffer", m, align="lstsq", clamp=False, min_depth=0.25)
    assert same_floats(loose, dict(zip(gm.ALIGNED_DEPTH_FIELDS[1:], run(p, t, m, "lstsq", False, 0.25)[0][-1, 1:].cpu().tolist())))


def test_accumulator_with_align_is_mean_and_sample_std_of_the_image_rows():
    a, b = case(2, 37, 53), case(3, 37, 53, seed=12)
    mb = b[2].clone()
    mb[1] = False                                             # an empty image is left out
    acc = gm.MetricsAccumulator("depth_zbuffer", align="lstsq")
    acc.update(*a)
    acc.update(b[0], b[1], mb)
    got = acc.compute()
    rows = torch.cat([run(*a, "lstsq")[0][:2], run(b[0], b[1], mb, "lstsq")[0][:3]]).cpu()
    rows = rows[rows[:, 0] > 0].numpy()
    assert got["num_images"] == 4 == len(rows) and set(got) == set(gm.ALIGNED_DEPTH_FIELDS) | {"num_images"}
    for k, name in enumerate(gm.ALIGNED_DEPTH_FIELDS):
        mean, std = got[name]
        assert abs(mean - rows[:, k].mean()) <= 1e-12 * max(1.0, abs(mean)), name
        assert abs(std - rows[:, k].std(ddof=1)) <= 1e-7 * max(1.0, abs(rows[:, k].mean())), name


def test_eval_checkpoint_align_on_a_synthetic_depth_checkpoint(tmp_path, monkeypatch):
    """tools/eval_checkpoint.py --task depth --align lstsq on the synthetic checkpoint of test_gpu_eval_checkpoint.py: the
    report's metrics are aligned_depth_metrics of the very tensors the tool evaluated, with the alignment summary."""
    from PIL import Image

    from omnidata_amd.weights import random_state_dict
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eval_checkpoint as ec
    ckpt = tmp_path / "omnidata_dpt_depth_v2.ckpt"
    torch.save({"state_dict": {"model." + k: v for k, v in random_state_dict(0, 1).items()}}, ckpt)
    img_dir, gt_dir = tmp_path / "img", tmp_path / "gt"
    img_dir.mkdir()
    gt_dir.mkdir()
    rng = np.random.default_rng(0)
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (400, 480 + 16 * i, 3), dtype=np.uint8)).save(img_dir / f"im{i}.png")
        np.save(gt_dir / f"im{i}.npy", rng.random((400, 480 + 16 * i)).astype(np.float32))
    seen = []
    real = gm.aligned_depth_metrics

    def spy(pred, target, mask, **kw):
        seen.append((pred.clone(), target.clone(), mask.clone(), kw))
        return real(pred, target, mask, **kw)
    monkeypatch.setattr(gm, "aligned_depth_metrics", spy)
    out = tmp_path / "report.json"
    ec.main(["--task", "depth", "--ckpt", str(ckpt), "--images", str(img_dir), "--gt", str(gt_dir), "--dtypes", "mixed", "--batch", "2",
             "--align", "lstsq", "--out", str(out)])
    entry = json.loads(out.read_text())["dtypes"]["mixed"]
    assert len(seen) == 1 and seen[0][3]["align"] == "lstsq" and entry["metrics_images"] == 2
    pred, tgt, msk, _ = seen[0]
    d, co = real(pred, tgt, msk, align="lstsq", return_coeffs=True)
    assert set(entry["metrics"]) == set(gm.ALIGNED_DEPTH_FIELDS[1:])
    for k, v in entry["metrics"].items():
        assert v == float(d[k]) or (np.isnan(v) and np.isnan(float(d[k]))), k
    co = co.double().cpu()
    assert entry["alignment"]["mode"] == "lstsq"
    for k, name in enumerate(("scale", "shift")):
        assert entry["alignment"][name] == {"mean": float(co[:, k].mean()), "min": float(co[:, k].min()), "max": float(co[:, k].max())}
    with pytest.raises(SystemExit):
        ec.main(["--task", "normal", "--ckpt", str(ckpt), "--images", str(img_dir), "--align", "median"])
    with pytest.raises(ValueError):
        ec.evaluate("normal", str(ckpt), [str(img_dir / "im0.png")], align="lstsq")
