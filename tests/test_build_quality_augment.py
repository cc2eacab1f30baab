"""Static checks on the compiled gfx950 code object of the training augmentations (csrc/augment.hip; hipcc cross-compiles, no GPU
needed), from the code object's metadata only: every kernel without scratch and without spills, at most 128 VGPRs (four waves
per SIMD), the chain kernels' LDS -- one buffer of (32 + 14) x (64 + 14) floats per stage that hands its result on -- within
64 KB a block, and no LDS for the gather."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omnidata_amd", "csrc")
BUFFER = (32 + 14) * (64 + 14) * 4


def _metadata(src, tmp_path):
    from omnidata_amd.build import SOURCE_FLAGS, SOURCES
    assert src in SOURCES and "-packed-fp32-ops" in SOURCE_FLAGS[src]
    out = tmp_path / (src + ".s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17"] + SOURCE_FLAGS[src] +
                       ["-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, src)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    meta = {}
    for block in out.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", block, flags=re.M).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"^\s+\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|"
                                                       r"group_segment_fixed_size|vgpr_count):\s+(\d+)", block, flags=re.M)}
    return meta


def test_augment_kernels_compile_without_scratch_or_spills_and_fit_four_waves_per_simd(tmp_path):
    meta = _metadata("augment.hip", tmp_path)
    chain = [n for n in meta if "augment_chain_kernel" in n]
    gather = [n for n in meta if "augment_gather_kernel" in n]
    assert len(chain) == 7 and len(gather) == 1 and len(meta) == 8       # one chain kernel per non-empty set of stages
    for n, m in meta.items():
        print(n, m)
        assert len(m) == 5, (n, m)
        assert m["private_segment_fixed_size"] == 0, (n, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
        assert m["vgpr_count"] <= 128, (n, m)
    lds = sorted(meta[n]["group_segment_fixed_size"] for n in chain)
    assert lds == [BUFFER] * 3 + [2 * BUFFER] * 3 + [3 * BUFFER], lds      # one stage, two stages, all three
    assert lds[-1] <= 64 * 1024
    assert meta[gather[0]]["group_segment_fixed_size"] == 0
