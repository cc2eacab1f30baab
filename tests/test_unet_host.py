"""The version-1 UNet without a GPU: the restatement against the reference's goldens, the packed-blob layout through a
host-only handle, strict loading, the CLI's choices and the compiled kernels' register budget."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.unet_restatement import (GOLDEN_CASES, load_golden, unet_forward_fp32, unet_input, unet_random_state_dict,
                                    unet_state_dict_spec)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def test_spec_has_the_references_174_keys():
    from omnidata_amd.unet import unet_state_dict_spec as engine_side_spec
    spec = unet_state_dict_spec(3)
    assert len(spec) == 174 and len({k for k, _ in spec}) == 174
    assert list(engine_side_spec(3).items()) == [(k, tuple(s)) for k, s in spec]
    d = dict(spec)
    assert d["down1.conv1.weight"] == (16, 3, 3, 3) and d["down_blocks.3.bn2.bias"] == (256,) and d["mid_conv1.weight"] == (1024, 1024, 3, 3)
    assert d["bn1.weight"] == (1024,) and d["up_blocks.5.conv1.weight"] == (512, 1536, 3, 3) and d["last_conv2.bias"] == (3,)
    assert sum(int(np.prod(s)) for _, s in spec) == 75_529_971   # the 75.5 M parameters of the v1 checkpoint


@pytest.mark.parametrize("name", [n for n, c in GOLDEN_CASES.items() if max(c[3], c[4]) <= 192])
def test_restatement_matches_reference_golden(name):
    """unet_forward_fp32 against the reference's own module (tools/make_unet_golden.py).  Same arithmetic, so only fp32
    reassociation separates them: each of the L = 45 convolutions adds a relative error of at most a few units of
    u = 2^-24 per output (blocked fp32 summation: ~log2(K) u sum|a||w|, and sum|a||w| / |out| stays below ~4 for these
    He-scaled, normalised layers: 8 u in all), every GroupNorm renormalises what came before it instead of amplifying it, and
    the errors of successive layers add: L * 8 u of the output range, 2.1e-5 of it."""
    seed, oc, B, H, W = GOLDEN_CASES[name]
    g = load_golden(GOLDEN, name)
    assert (int(g["seed"]), int(g["out_channels"])) == (seed, oc) and tuple(g["shape"]) == (B, oc, H, W)
    y = unet_forward_fp32(unet_random_state_dict(seed, oc), unet_input(seed, B, H, W)).numpy()
    rng = float(g["y"].max() - g["y"].min())
    bound = 45 * 8 * 2.0 ** -24 * rng
    err = float(np.abs(y - g["y"]).max())
    print(f"{name}: max |restatement - golden| = {err:.3e}, bound {bound:.3e} (range {rng:.2f})")
    assert err <= bound
    assert 0 < float(g["e_model_fp16"]) < float(g["e_model_bf16"]) < 0.25 * rng


@pytest.fixture(scope="module")
def packed(built_lib):
    from omnidata_amd.unet import UNetEngine
    out = {}
    sd = unet_random_state_dict(5, 3)
    for dtype in ("fp16", "bf16"):
        e = UNetEngine(out_channels=3, max_batch=1, dtype=dtype, device_id=None, max_hw=(64, 64))
        e.load_state_dict(sd)
        out[dtype] = (e, e.export_packed_host())
    yield sd, out
    for e, _ in out.values():
        e.close()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_packed_blob_layout(packed, dtype):
    sd, handles = packed
    e, blob = handles[dtype]
    tdt = TDT[dtype]
    assert blob.size == e.packed_bytes and e.device_bytes == 0

    def entry16(key):
        off, n = e.packed_entry(key)
        assert off % 256 == 0
        return torch.from_numpy(blob[off:off + n].copy()).view(tdt).float()

    def entry32(key):
        off, n = e.packed_entry(key)
        return torch.from_numpy(blob[off:off + n].copy()).view(torch.float32)

    # entries follow the state-dict order, 256-byte aligned, nothing overlaps
    end = 0
    for k, _ in unet_state_dict_spec(3):
        off, n = e.packed_entry(k)
        assert off == end and n > 0, k
        end = (off + n + 255) // 256 * 256
    assert end == blob.size
    # the first layer: one padded k-block of 32, k = (ky*3 + kx)*3 + c, k = 27..31 zero
    w = sd["down1.conv1.weight"]
    got = entry16("down1.conv1.weight").reshape(16, 32)
    want = torch.zeros(16, 32)
    want[:, :27] = w.permute(0, 2, 3, 1).reshape(16, 27).to(tdt).float()
    assert torch.equal(got, want)
    # a 96 -> 32 and a 1536 -> 512 layer: [O][ky][kx][I], I in torch.cat's order (up-sampled channels first, then the skip)
    for k in ("up_blocks.1.conv1.weight", "up_blocks.5.conv1.weight"):
        w = sd[k]
        want = w.permute(0, 2, 3, 1).contiguous().to(tdt).float()
        got = entry16(k).reshape(want.shape)
        assert torch.equal(got, want), k
        c = w.shape[0]   # c_i; the up-sampled tensor has 2 c_i channels, the skip c_i
        assert torch.equal(got[..., :2 * c], w[:, :2 * c].permute(0, 2, 3, 1).to(tdt).float())
        assert torch.equal(got[..., 2 * c:], w[:, 2 * c:].permute(0, 2, 3, 1).to(tdt).float())
    # fp32 vectors and the 1x1 head verbatim
    for k in ("up_blocks.1.conv1.bias", "down_blocks.3.bn2.bias", "bn1.weight", "last_conv2.weight", "last_conv2.bias"):
        assert torch.equal(entry32(k), sd[k].flatten()), k


def test_strict_loading(built_lib):
    from omnidata_amd.unet import UNet, UNetEngine
    sd = unet_random_state_dict(0, 3)
    e = UNetEngine(out_channels=3, max_batch=1, device_id=None, max_hw=(64, 64))
    assert e.load_tensor("not.a.key", torch.zeros(1)) == -2                         # DPTX_E_KEY
    assert e.load_tensor("last_conv2.bias", torch.zeros(1)) == -2                   # out_channels = 3 expects [3]
    assert e.load_tensor("down1.conv1.weight", torch.zeros(16, 3, 3)) == -2
    with pytest.raises(RuntimeError, match="shape mismatch"):
        e.load_state_dict({"last_conv2.bias": torch.zeros(1)})
    partial = {k: v for k, v in sd.items() if k not in ("down_blocks.3.bn2.bias", "mid_conv2.weight")}
    with pytest.raises(RuntimeError, match=r"missing tensors \(2\).*down_blocks\.3\.bn2\.bias.*mid_conv2\.weight"):
        e.load_state_dict(partial)
    with pytest.raises(RuntimeError, match="not finalized"):
        e.export_packed_host()
    e.load_state_dict(sd)
    plain = e.export_packed_host()
    # the checkpoint form of the reference's demo.py: {'state_dict': {'model.<key>': tensor}}
    e2 = UNetEngine(out_channels=3, max_batch=1, device_id=None, max_hw=(64, 64))
    e2.load_state_dict({"state_dict": {"model." + k: v for k, v in sd.items()}})
    assert np.array_equal(plain, e2.export_packed_host())
    m = UNet(out_channels=3)
    m.load_state_dict({"state_dict": {"model." + k: v for k, v in sd.items()}})
    assert list(m.state_dict().keys()) == list(sd.keys()) and all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError):
        m.load_state_dict(partial)
    # a host-only handle has no forward
    rc = e.lib.dptx_unet_forward(e.h, 1, 1, 1, 64, 64, 0, None)
    assert rc == -4
    e.close()
    e2.close()


def test_config_limits(built_lib):
    from omnidata_amd.unet import UNetEngine
    for dtype in ("bf16x3", "fp16x3", "mixed", "fp8"):   # the plane dtypes and fp8
        with pytest.raises(RuntimeError, match="invalid"):
            UNetEngine(dtype=dtype, device_id=None)
    for kw in (dict(max_hw=(96, 64)), dict(max_hw=(64, 576)), dict(max_hw=(32, 64)), dict(max_batch=33), dict(max_batch=0),
               dict(out_channels=5), dict(out_channels=0)):
        with pytest.raises(RuntimeError, match="invalid"):
            UNetEngine(device_id=None, **kw)
    for oc in (1, 4):
        e = UNetEngine(out_channels=oc, device_id=None, max_hw=(512, 512), max_batch=32, dtype="bf16")
        assert e.packed_entry("last_conv2.weight")[1] == oc * 16 * 4
        e.close()


def test_python_model_rejects_bad_sizes_and_cpu():
    from omnidata_amd.unet import UNet
    m = UNet(out_channels=1, max_size=128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 64, 64))
    for kw in (dict(downsample=5), dict(in_channels=1)):
        with pytest.raises(NotImplementedError):
            UNet(**kw)
    with pytest.raises(ValueError):
        UNet(dtype="mixed")


def test_demo_help_lists_unet():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo.py"), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    m = re.search(r"--backbone \{([^}]*)\}", r.stdout)
    assert m and "unet" in m.group(1).split(",") and "vitb_rn50_384" in m.group(1)


def test_unet_kernels_build_without_spills(tmp_path):
    """unet.hip is part of the library, built without packed fp32 arithmetic like the other VALU sources; no kernel uses
    scratch memory, and the small-channel convolution runs on the 32x32x16 MFMA in both element types."""
    from omnidata_amd.build import SOURCE_FLAGS, SOURCES
    assert "unet.hip" in SOURCES and "unet_engine.hip" in SOURCES and "-packed-fp32-ops" in SOURCE_FLAGS["unet.hip"]
    out = tmp_path / "unet.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17"] + SOURCE_FLAGS["unet.hip"] +
                       ["-S", "--cuda-device-only", "-o", str(out), os.path.join(ROOT, "omnidata_amd", "csrc", "unet.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    s = out.read_text()
    names = re.findall(r"^\s+\.name:\s+(\S+)", s, flags=re.M)
    priv = re.findall(r"^\s+\.private_segment_fixed_size:\s+(\d+)", s, flags=re.M)
    spills = re.findall(r"^\s+\.vgpr_spill_count:\s+(\d+)", s, flags=re.M)
    lds = re.findall(r"^\s+\.group_segment_fixed_size:\s+(\d+)", s, flags=re.M)
    assert len(names) >= 25 and len(priv) == len(names) == len(spills)
    assert sum("unet_conv_small_kernel" in n for n in names) == 14      # 7 (Cin, Cout) classes x 2 element types
    assert all(int(p) == 0 for p in priv), dict(zip(names, priv))
    assert all(int(p) == 0 for p in spills) and "scratch_" not in s
    assert all(int(v) <= 160 * 1024 for v in lds)
    assert "v_mfma_f32_32x32x16_f16" in s and "v_mfma_f32_32x32x16_bf16" in s
    bad = [ln for ln in s.splitlines() if re.search(r"\bv_pk_\w+_f32\b", ln) and re.search(r"op_sel:\[[01,]*1", ln)]
    assert not bad
