"""Static checks on the compiled gfx950 code object of the streaming 1x1 kernel (csrc/conv1x1.hip; hipcc cross-compiles, no
GPU needed): no scratch, no spills, and the instructions its design rests on."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omnidata_amd", "csrc")


def test_conv1x1_no_scratch_no_spills_mfma_and_lds_dma(tmp_path):
    from omnidata_amd.build import SOURCE_FLAGS
    out = tmp_path / "conv1x1.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17"] + SOURCE_FLAGS.get("conv1x1.hip", []) +
                       ["-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "conv1x1.hip")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    s = out.read_text()
    names = re.findall(r"^\s+\.name:\s+(\S+)", s, flags=re.M)
    priv = re.findall(r"^\s+\.private_segment_fixed_size:\s+(\d+)", s, flags=re.M)
    spills = re.findall(r"^\s+\.vgpr_spill_count:\s+(\d+)", s, flags=re.M)
    assert names and len(priv) == len(names) and len(spills) == len(names)
    assert all(int(p) == 0 for p in priv), dict(zip(names, priv))
    assert all(int(p) == 0 for p in spills), dict(zip(names, spills))
    assert "v_mfma_f32_32x32x16_bf16" in s and "v_mfma_f32_32x32x16_f16" in s
    assert re.search(r"buffer_load_dwordx4 .* lds", s), "direct-to-LDS staging missing"
