"""Static checks on the compiled gfx950 code object of tiled inference (csrc/tiles.hip; hipcc cross-compiles, no GPU needed), from
the code object's metadata only: every kernel without scratch and without spills, no LDS beyond the uint8 row staging of the
blend (and block_sum's 16 doubles in the shared stats pass), and few enough VGPRs for at least four waves per SIMD."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omnidata_amd", "csrc")
ROW_STAGING = 4 * (3 * 64 // 4 + 4) * 4     # resample_batch.h: TH rows of row_dw(TW) dwords


def _metadata(src, tmp_path):
    from omnidata_amd.build import HEADERS, SOURCE_FLAGS, SOURCES
    assert src in SOURCES and "-packed-fp32-ops" in SOURCE_FLAGS[src] and "tta_depth_align.h" in HEADERS
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


def test_tile_kernels_compile_without_scratch_or_spills_and_fit_four_waves_per_simd(tmp_path):
    meta = _metadata("tiles.hip", tmp_path)
    kinds = {k: [n for n in meta if k in n] for k in ("tile_blend_normals_kernel", "tile_blend_depth_kernel", "tta_depth_anchor_kernel",
                                                      "tta_depth_stats_kernel", "tta_depth_solve_kernel")}
    assert [len(v) for v in kinds.values()] == [2, 1, 1, 1, 1] and len(meta) == 6         # normals: uint8 and fp32
    for n, m in meta.items():
        assert len(m) == 5, (n, m)
        assert m["private_segment_fixed_size"] == 0, (n, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (n, m)
        assert m["vgpr_count"] <= 128, (n, m)                                             # 512 / 128: four waves per SIMD
    lds = {k: max(meta[n]["group_segment_fixed_size"] for n in v) for k, v in kinds.items()}
    assert lds["tile_blend_normals_kernel"] == ROW_STAGING == 832
    assert min(meta[n]["group_segment_fixed_size"] for n in kinds["tile_blend_normals_kernel"]) <= 4   # fp32: no staging
    assert lds["tile_blend_depth_kernel"] == 0 and lds["tta_depth_anchor_kernel"] == 0 and lds["tta_depth_solve_kernel"] == 0
    assert lds["tta_depth_stats_kernel"] == 128                                           # block_sum's 16 doubles
    for n in kinds["tile_blend_normals_kernel"] + kinds["tile_blend_depth_kernel"]:
        assert meta[n]["vgpr_count"] <= 64, (n, meta[n])                                  # eight waves: the taps' latency is hidden by occupancy


def test_the_alignment_kernels_have_the_same_resources_in_both_units(tmp_path):
    """tta_depth.hip and tiles.hip compile the same header: the shared kernels come out alike (the GPU tests compare their bits)"""
    a, b = _metadata("tiles.hip", tmp_path), _metadata("tta_depth.hip", tmp_path)
    for kind in ("tta_depth_anchor_kernel", "tta_depth_stats_kernel", "tta_depth_solve_kernel"):
        (na,), (nb,) = [n for n in a if kind in n], [n for n in b if kind in n]
        assert na == nb and a[na] == b[nb], kind
