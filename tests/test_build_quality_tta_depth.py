"""Static checks on the compiled gfx950 code object of the depth alignment and merge of test-time augmentation
(csrc/tta_depth.hip; hipcc cross-compiles, no GPU needed): every kernel without scratch and without spills, the stats pass
light enough for eight waves per SIMD (its latency is hidden by occupancy), and no packed fp32 arithmetic."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omnidata_amd", "csrc")


def _compile(src, tmp_path):
    from omnidata_amd.build import HEADERS, SOURCE_FLAGS, SOURCES
    assert src in SOURCES and "-packed-fp32-ops" in SOURCE_FLAGS[src] and "tta_common.h" in HEADERS
    out = tmp_path / (src + ".s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17"] + SOURCE_FLAGS[src] +
                       ["-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, src)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    s = out.read_text()
    meta = {}
    for block in s.split("  - .agpr_count:")[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", block, flags=re.M).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"^\s+\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|"
                                                       r"group_segment_fixed_size|vgpr_count):\s+(\d+)", block, flags=re.M)}
    return s, meta


def test_tta_depth_kernels_compile_without_scratch_or_spills(tmp_path):
    s, meta = _compile("tta_depth.hip", tmp_path)
    kinds = {k: [n for n in meta if k in n] for k in ("tta_depth_anchor_kernel", "tta_depth_stats_kernel", "tta_depth_solve_kernel",
                                                      "tta_depth_merge_kernel")}
    assert [len(v) for v in kinds.values()] == [1, 1, 1, 5] and len(meta) == 8     # merge: mean + the classes of 8 / 16 / 32 / 64 views
    for n, m in meta.items():
        assert len(m) == 5, (n, m)
        assert m["private_segment_fixed_size"] == 0, (n, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
        assert m["group_segment_fixed_size"] <= 1024, (n, m)                      # block_sum's 16 doubles, nothing else
        assert m["vgpr_count"] <= 128, (n, m)
    assert meta[kinds["tta_depth_stats_kernel"][0]]["vgpr_count"] <= 64           # eight waves per SIMD
    assert not re.search(r"\bscratch_", s)
    assert not re.search(r"v_pk_\w+_f32", s)
