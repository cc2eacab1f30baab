"""The version-1 UNet end to end on the GPU: the whole forward against the reference's goldens (tools/make_unet_golden.py),
the invariances of the engine, and the Python / CLI surface.  pytest -m gpu.

Measured ratios max |gpu - golden| / e_model are printed by test_forward_matches_reference_golden and recorded in
profiles/unet_parity.md."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from tests.unet_restatement import GOLDEN_CASES, load_golden, unet_input, unet_random_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"


@functools.lru_cache(maxsize=2)
def seeded(seed, oc):
    return unet_random_state_dict(seed, oc)


def make_engine(seed, oc, dtype, max_batch=3, max_hw=(384, 384)):
    from omnidata_amd.unet import UNetEngine
    e = UNetEngine(out_channels=oc, max_batch=max_batch, dtype=dtype, device_id=0, max_hw=max_hw)
    e.load_state_dict(seeded(seed, oc))
    return e


@pytest.mark.parametrize("name", list(GOLDEN_CASES))
def test_forward_matches_reference_golden(name):
    """max |gpu - golden| <= 2 x e_model_<dtype> of the golden file, both dtypes.  e_model is the distance of the CPU rounding
    model (tests/unet_restatement.py unet_forward_rounded) from the reference's fp32 output on the same input; the factor 2 is
    the margin for the GPU's summation order inside the MFMA and across k, each flipped rounding being one more error of the
    size the model already counts."""
    seed, oc, B, H, W = GOLDEN_CASES[name]
    g = load_golden(GOLDEN, name)
    x = unet_input(seed, B, H, W).to(DEV)
    want = torch.from_numpy(g["y"]).to(DEV)
    ratios = {}
    for dtype in ("fp16", "bf16"):
        e = make_engine(seed, oc, dtype, max_batch=B, max_hw=(H, W))
        y = e.forward(x)
        assert not e.range_overflowed()
        e.close()
        assert y.shape == want.shape and y.dtype == torch.float32 and torch.isfinite(y).all()
        err = float((y - want).abs().max())
        ratios[dtype] = err / float(g[f"e_model_{dtype}"])
        print(f"\n[unet parity] {name} {dtype}: max |gpu - golden| {err:.4e}, e_model {float(g[f'e_model_{dtype}']):.4e}, "
              f"ratio {ratios[dtype]:.3f}")
    assert all(r <= 2.0 for r in ratios.values()), ratios


@pytest.fixture(scope="module")
def engine0():
    e = make_engine(0, 3, "fp16")
    yield e
    e.close()


def test_invariances_bitwise(engine0):
    """Image i of a batch of 3 equals the same image run alone; two runs agree; a run after the arena was filled with 0xFF
    (NaN in every element type) agrees; 64x64 after a 128x192 call on the same handle equals 64x64 on a fresh handle."""
    e = engine0
    x = unet_input(7, 3, 64, 64).to(DEV)
    y3 = e.forward(x)
    assert torch.isfinite(y3).all()
    for i in range(3):
        assert torch.equal(e.forward(x[i:i + 1]), y3[i:i + 1]), i
    assert torch.equal(e.forward(x), y3)
    torch.cuda.synchronize()
    e.arena_fill(0xFF)
    assert torch.equal(e.forward(x), y3)
    big = e.forward(unet_input(8, 1, 128, 192).to(DEV))
    assert torch.isfinite(big).all()
    after = e.forward(x)
    fresh = make_engine(0, 3, "fp16")
    assert torch.equal(fresh.forward(x), after) and torch.equal(after, y3)
    fresh.close()
    # 16-bit inputs are read directly: the same values give the same bits
    xh = x.half()
    assert torch.equal(e.forward(xh), e.forward(xh.float()))
    xb = x.bfloat16()
    assert torch.equal(e.forward(xb), e.forward(xb.float()))


def test_forward_rejects_bad_sizes(engine0):
    e = engine0
    for shape in ((1, 3, 96, 64), (1, 3, 64, 32), (1, 3, 448, 64), (4, 3, 64, 64)):
        with pytest.raises(RuntimeError, match="invalid"):
            e.forward(torch.zeros(*shape, device=DEV))
    assert not e.range_overflowed()


def test_range_flag_and_bf16_fallback():
    """Weights that push a raw convolution output beyond 65504: the fp16 engine's statistics set the flag; the model warns
    once and continues in bf16, whose result is finite."""
    from omnidata_amd.unet import UNet
    sd = {k: v.clone() for k, v in seeded(0, 3).items()}
    sd["down1.conv2.weight"] *= 3.0e5
    m = UNet(out_channels=3, max_batch=2, max_size=64)
    m.load_state_dict(sd)
    m.to(DEV)
    x = unet_input(1, 2, 64, 64).to(DEV)
    with pytest.warns(UserWarning, match="switching this model to dtype='bf16'"):
        y = m(x)
    assert m.engine_dtype == "bf16" and torch.isfinite(y).all()
    y2 = m(x)
    assert torch.equal(y, y2)


def test_python_surface(engine0, tmp_path):
    from omnidata_amd.batch_infer import BatchPredictor
    from omnidata_amd.normal_loss import NormalLoss, _normal_inputs
    from omnidata_amd.unet import UNet
    sd = seeded(0, 3)
    x = unet_input(9, 2, 64, 128).to(DEV)
    want = engine0.forward(x)
    m = UNet(out_channels=3, max_batch=2, max_size=384)
    m.load_state_dict(sd)
    m.to(DEV)
    y = m(x)
    assert torch.equal(y, want)                                   # the C-ABI result, bit for bit
    assert list(m.state_dict().keys()) == list(sd.keys())
    m2 = UNet(out_channels=3, max_batch=1, max_size=384)          # the checkpoint form of the reference's demo.py; chunked batch
    m2.load_state_dict({"state_dict": {"model." + k: v for k, v in sd.items()}})
    m2.to(DEV)
    assert torch.equal(m2(x), want)
    # the result feeds the normal objective as it is: fp32, contiguous, no copy
    gt = torch.rand(2, 3, 64, 128, device=DEV)
    mask = torch.ones(2, 1, 64, 128, dtype=torch.bool, device=DEV)
    p, _, _ = _normal_inputs(y, gt, mask)
    assert p.data_ptr() == y.data_ptr()
    out = NormalLoss()(y, gt, mask)
    assert all(torch.isfinite(v) for v in out.values())
    # BatchPredictor over three small PNGs: the pixels of three single calls
    rng = np.random.default_rng(3)
    files = []
    for i, (h, w) in enumerate(((80, 100), (64, 64), (120, 90))):
        f = tmp_path / f"im{i}.png"
        Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(f)
        files.append(str(f))
    batched = [t.cpu() for t in BatchPredictor(m, "normal", batch_size=2, image_size=128).predict(files)]
    single = [next(iter(BatchPredictor(m, "normal", batch_size=1, image_size=128).predict([f]))).cpu() for f in files]
    assert len(batched) == 3 and all(b.shape == (128, 128, 3) and torch.equal(b, s) for b, s in zip(batched, single))


def test_demo_cli_unet(tmp_path):
    rng = np.random.default_rng(0)
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(rng.integers(0, 255, (200, 260, 3), dtype=np.uint8)).save(src / "test1.png")
    out = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo.py"), "--backbone", "unet", "--random-weights", "0", "--task", "normal",
                        "--img_path", str(src), "--output_path", str(out)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    img = Image.open(out / "test1_normal.png")
    assert img.size == (384, 384) and np.asarray(img).std() > 0
    assert (out / "test1_rgb.png").exists()
