"""Static checks on the compiled gfx950 code objects of the second stem form (csrc/stem.hip stem_conv_kernel_wp) and of the
strip form of the x2 up-sampling (csrc/misc.hip upsample2x_strip_kernel); hipcc cross-compiles, no GPU needed.  The stem form
exists to put four blocks on a CU: no scratch, and VGPRs and LDS such that four blocks of four waves fit.  The up-sampling
form: no scratch."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omnidata_amd", "csrc")
VGPRS_PER_SIMD = 512      # gfx950: unified vector register file per SIMD lane (ArchVGPRs + AccVGPRs)
LDS_PER_CU = 160 * 1024   # gfx950
LDS_GRANULE = 1280        # allocation granularity in bytes (320 dwords)


def kernel_metadata(tmp_path, src):
    """{kernel name: {field: int}} from the resource metadata hipcc writes into the assembly of omnidata_amd/csrc/<src>"""
    from omnidata_amd.build import SOURCE_FLAGS
    out = tmp_path / (src + ".s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17"] + SOURCE_FLAGS.get(src, []) +
                       ["-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, src)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    meta = {}
    for entry in re.split(r"^\s+- \.agpr_count:", out.read_text(), flags=re.M)[1:]:
        entry = ".agpr_count:" + entry
        name = re.search(r"^\s*\.name:\s+(\S+)", entry, flags=re.M)
        if name is None:
            continue
        fields = dict(re.findall(r"^\s*\.(agpr_count|vgpr_count|group_segment_fixed_size|private_segment_fixed_size|vgpr_spill_count|"
                                 r"sgpr_spill_count):\s+(\d+)", entry, flags=re.M))
        meta[name.group(1)] = {k: int(v) for k, v in fields.items()}
    return meta


def test_stem_wp_forms_no_scratch_and_four_blocks_per_cu(tmp_path):
    meta = {n: m for n, m in kernel_metadata(tmp_path, "stem.hip").items() if "stem_conv_kernel_wp" in n}
    assert len(meta) == 6, sorted(meta)   # bf16 / fp16 x caller image fp32 / bf16 / fp16
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        # four blocks of four waves per CU = four waves per SIMD
        assert 4 * m["vgpr_count"] <= VGPRS_PER_SIMD, (name, m)
        lds = -(-m["group_segment_fixed_size"] // LDS_GRANULE) * LDS_GRANULE
        assert 0 < lds and 4 * lds <= LDS_PER_CU, (name, m)


def test_upsample_strip_forms_no_scratch(tmp_path):
    meta = {n: m for n, m in kernel_metadata(tmp_path, "misc.hip").items() if "upsample2x_strip_kernel" in n}
    assert len(meta) == 4, sorted(meta)   # bf16 / fp16 x strips of 4 / 8 rows
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
